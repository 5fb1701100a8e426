#!/usr/bin/env python3
"""Time the IoU-Net box ascent (mmtrack_amd.iounet.AtomIoUNet.refine_boxes -> mmt_iounet_refine) on one MI355X.

Method (DESIGN.md section 9 "Timing"): HIP events, median of 50 runs of 20 back-to-back calls after 10 warm-ups.
Real head (256 pooled channels, 256 hidden units per level), P = 10 proposals, 5 iterations, full-size maps
(36 x 36 at 1/8 and 18 x 18 at 1/16), B = 1 and B = 32 sequences.  Also the four PrRoIPool launches of one iteration
(two forwards, two box gradients) on the same boxes, timed the same way: the launches of one iteration run one after
the other on one stream, so iteration time minus that is the time of the head's own kernels (box -> ROI, the two
row-linear launches, the head reduce, the two transposed launches, the box step).

Floors per iteration, printed beside the measurements: the two hidden layers' fp32 weights (8.9 MB) read twice
(forward and transposed) at --tbps, and 4 * rows * (6400 + 2304) * 256 FLOP at the 157 TF/s fp32-MFMA peak.

Usage:  python tools/bench_iounet.py [--tbps 4.0] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-modal-trakcing-bechmark_amd"))

from mmtrack_amd import _lib, synth  # noqa: E402
from mmtrack_amd.iounet import AtomIoUNet  # noqa: E402

RUNS, CALLS, WARM = 50, 20, 10
P, ITERS, SIZE = 10, 5, 288
PEAK_TF = 157.0


def timed(fn):
    """Median over RUNS of the time of one call (us), CALLS back-to-back calls per run."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tbps", type=float, default=4.0, help="memory rate of the weight floor, TB/s")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    net = AtomIoUNet(synth.make_iounet_state_dict(4, input_dim=(32, 32)), device=dev, precision="fp32")
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)
    res = {}
    for B in (1, 32):
        feat = [torch.randn(B, 256, SIZE // 8, SIZE // 8, generator=g).relu().to(dev).contiguous(memory_format=torch.channels_last),
                torch.randn(B, 256, SIZE // 16, SIZE // 16, generator=g).relu().to(dev).contiguous(memory_format=torch.channels_last)]
        mod = [(torch.rand(B, 256, generator=g) + 0.25).to(dev) for _ in range(2)]
        wh = SIZE * (0.2 + 0.4 * torch.rand(B, P, 2, generator=g))
        xy = (SIZE - wh) * torch.rand(B, P, 2, generator=g)
        boxes = torch.cat([xy, wh], dim=2).to(dev)
        # step 0: the boxes stay where they are, so every call does the same work
        t_refine = timed(lambda: net.refine_boxes(mod, feat, boxes, ITERS, 0.0, 1.0))
        R = B * P
        rois = torch.cat([torch.arange(B, dtype=torch.float32).repeat_interleave(P)[:, None].to(dev),
                          boxes.reshape(R, 4)[:, :2], boxes.reshape(R, 4)[:, :2] + boxes.reshape(R, 4)[:, 2:]], dim=1).contiguous()
        s = _lib.stream(dev)
        bufs = []
        for f, bins, scale in ((feat[0], 5, 1 / 8), (feat[1], 3, 1 / 16)):
            n, c, h, w = f.shape
            out = torch.empty(R, c, bins, bins, device=dev)
            bufs.append((f, (n, h, w, c, c, w * c, h * w * c), bins, scale, out, torch.randn(R, c, bins, bins, device=dev),
                         torch.empty(R, 5, device=dev)))

        def pools():
            for f, (n, h, w, c, pix, row, img), bins, scale, out, gout, groi in bufs:
                lib.mmt_prroi_pool_rois(_lib.ptr(f), n, h, w, c, pix, row, img, _lib.ptr(rois), R, scale, bins, bins,
                                        _lib.ptr(out), s)
            for f, (n, h, w, c, pix, row, img), bins, scale, out, gout, groi in bufs:
                lib.mmt_prroi_pool_rois_grad_rois(_lib.ptr(f), n, h, w, c, pix, row, img, _lib.ptr(rois), R, scale, bins,
                                                  bins, _lib.ptr(out), _lib.ptr(gout), _lib.ptr(groi), s)
        t_pool = timed(pools)
        weights = (6400 + 2304) * 256 * 4
        flop = 4.0 * R * (6400 + 2304) * 256
        res[f"B{B}"] = dict(rows=R, refine_us=t_refine, iteration_us=t_refine / ITERS, prroi_us=t_pool,
                            head_us=t_refine / ITERS - t_pool, floor_weights_us=2 * weights / (args.tbps * 1e6),
                            floor_mfma_us=flop / (PEAK_TF * 1e6))
    if args.json:
        print(json.dumps(res))
        return
    for k, r in res.items():
        print(f"{k}: {r['rows']} rows  refine_boxes({ITERS} iterations) {r['refine_us']:.1f} us = {r['iteration_us']:.1f} us per "
              f"iteration; its four PrRoIPool launches {r['prroi_us']:.1f} us; the head's own kernels {r['head_us']:.1f} us "
              f"(floors: weights twice at {args.tbps} TB/s {r['floor_weights_us']:.1f} us, MFMA {r['floor_mfma_us']:.1f} us)")


if __name__ == "__main__":
    main()
