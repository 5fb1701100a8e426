"""IoU-Net for DeT's ``ltr`` on an MI355X: the name the reference exports from this package, served by the HIP predictor
of mmtrack_amd.iounet (the package directory of mmtrack_amd must be on sys.path)."""
from mmtrack_amd.iounet import AtomIoUNet

__all__ = ["AtomIoUNet"]
