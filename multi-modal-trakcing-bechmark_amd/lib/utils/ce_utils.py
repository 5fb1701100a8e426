"""Candidate-elimination template mask (ViPT/lib/utils/ce_utils.py:7-65): which template tokens' attention rows
score the search tokens.  All four values of MODEL.BACKBONE.CE_TEMPLATE_RANGE, with the reference's return values:
None for ALL, a bool [bs, Lz] mask for CTR_POINT / CTR_REC / GT_BOX, NotImplementedError where it raises one.  The
engine takes the CTR_POINT token as an index and every other range as a per-slot mask
(mmtrack_amd.Engine.set_ce_template_mask)."""

RANGES = ('ALL', 'CTR_POINT', 'CTR_REC', 'GT_BOX')
# template feature size -> the centre block's [start, stop) on both axes (ce_utils.py:23-46); a size missing here
# is the reference's NotImplementedError
_CTR_POINT = {8: (3, 4), 12: (5, 6), 7: (3, 4), 14: (6, 7)}
_CTR_REC = {8: (3, 5), 12: (5, 7), 7: (3, 4)}


def ctr_point_index(template_size: int, stride: int = 16) -> int:
    tf = template_size // stride
    if tf not in _CTR_POINT:
        raise NotImplementedError
    i = _CTR_POINT[tf][0]
    return i * tf + i


def template_mask(rng, template_size, stride, bs, device, gt_bbox=None):
    """generate_mask_cond on plain values.  gt_bbox: [bs, 4] x, y, w, h of the target in the template crop,
    normalised by the template size (GT_BOX only)."""
    import torch
    import torch.nn.functional as F
    tf = template_size // stride
    if rng == 'ALL':
        return None
    if rng in ('CTR_POINT', 'CTR_REC'):
        table = _CTR_POINT if rng == 'CTR_POINT' else _CTR_REC
        if tf not in table:
            raise NotImplementedError
        a, b = table[tf]
        m = torch.zeros([bs, tf, tf], device=device)
        m[:, a:b, a:b] = 1
        return m.flatten(1).to(torch.bool)
    if rng == 'GT_BOX':
        # the box rasterised at template resolution with int() slicing -- rows int(y) : int(y + h - 1), columns
        # int(x) : int(x + w - 1), negative bounds counting from the far edge as Python slices do --, then the
        # bilinear 1 / stride down-sampling; a token is in the mask where the result is non-zero (ce_utils.py:7-12,
        # 51-59)
        m = torch.zeros([bs, template_size, template_size], device=device)
        px = gt_bbox * template_size
        for i in range(bs):
            x, y, w, h = px[i].cpu().tolist()
            m[i, int(y):int(y + h - 1), int(x):int(x + w - 1)] = 1
        m = F.interpolate(m.unsqueeze(1).to(torch.float), scale_factor=1. / stride, mode='bilinear',
                          align_corners=False)
        return m.flatten(1).to(torch.bool)
    raise NotImplementedError


def generate_mask_cond(cfg, bs, device, gt_bbox):
    return template_mask(cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE, cfg.DATA.TEMPLATE.SIZE, cfg.MODEL.BACKBONE.STRIDE, bs,
                         device, gt_bbox)


def template_box_in_crop(init_bbox, resize_factor, template_size):
    """The init box in its own template crop, normalised: BaseTracker.transform_bbox_to_crop(init_bbox,
    resize_factor) (basetracker.py:38-57) = transform_image_to_crop(box, box, resize_factor, crop_sz, normalize=True)
    (processing_utils.py:86-109), with its tensor types.  Returns [1, 4], what ViPTTrack.initialize hands to
    generate_mask_cond (vipt.py:52-54)."""
    import torch
    crop_sz = torch.Tensor([template_size, template_size])
    box = torch.tensor(init_bbox)
    centre = box[0:2] + 0.5 * box[2:4]
    out_centre = (crop_sz - 1) / 2 + (centre - centre) * resize_factor
    out_wh = box[2:4] * resize_factor
    out = torch.cat((out_centre - 0.5 * out_wh, out_wh)) / crop_sz[0]
    return out.view(1, 4)
