"""SiamFC frames/s: the sequential tracker against SiamFCPool, in one process.

Seeded synthetic 480 x 640 x 3 sequences, frames resident on the device.  Every configuration is warmed up, then
the configurations alternate: TrackerSiamFC.update alone, SiamFCPool.update at B = 1, 8, 32 and
SiamFCPool.submit / fetch (one frame in flight) at the same B, each for at least --seconds, the whole round
repeated --repeats times.  A host clock around work that ends in a synchronise (update's read-back, fetch's event,
a final torch.cuda.synchronize()).  Prints one JSON line per configuration: the median frames/s of the repeats with
their minimum and maximum.  A pool is only ever compared with the sequential tracker of the same run.

  python tools/siamfc_pool_bench.py [--batches 1,8,32] [--seconds 1.0] [--repeats 3] [--frames 24]
  python tools/siamfc_pool_bench.py --profile 32     # 13 steps at B = 32 and 13 sequential ones, for a kernel trace
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "multi-modal-trakcing-bechmark_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sequences(n, frames):
    from mmtrack_amd.workspace import synthetic_sequences
    out = []
    for name, fr, gt in synthetic_sequences(n, frames, C=3):
        out.append((torch.from_numpy(fr).cuda(), list(gt[0])))
    return out


class Sequential:
    name, per_step = "sequential", 1

    def __init__(self, sd, seqs):
        from mmtrack_amd.siamfc import TrackerSiamFC
        self.tr, (self.frames, self.box) = TrackerSiamFC(state_dict=sd), seqs[0]
        self.reset()

    def reset(self):
        self.tr.init(self.frames[0], self.box)
        self.t = 1

    def step(self):
        if self.t == len(self.frames):
            self.reset()
        self.tr.update(self.frames[self.t])
        self.t += 1

    def drain(self):
        pass


class Pooled:
    def __init__(self, sd, seqs, B, pipelined):
        from mmtrack_amd.siamfc import SiamFCPool
        self.name, self.per_step = f"pool B={B} " + ("submit/fetch" if pipelined else "update"), B
        self.pool, self.seqs, self.pipelined, self.pend = SiamFCPool(sd, B), seqs[:B], pipelined, None
        self.reset()

    def reset(self):
        self.drain()
        for k, (frames, box) in enumerate(self.seqs):
            self.pool.init(k, frames[0], box)
        self.t = 1

    def step(self):
        if self.t == len(self.seqs[0][0]):
            self.reset()
        fr = [frames[self.t] for frames, _ in self.seqs]
        if self.pipelined:
            ticket = self.pool.submit(fr)
            if self.pend is not None:
                self.pool.fetch(self.pend)
            self.pend = ticket
        else:
            self.pool.update(fr)
        self.t += 1

    def drain(self):
        if self.pend is not None:
            self.pool.fetch(self.pend)
            self.pend = None


def timed(cfg, seconds):
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while True:
        cfg.step()
        steps += 1
        if time.perf_counter() - t0 >= seconds:
            break
    cfg.drain()
    torch.cuda.synchronize()
    return steps * cfg.per_step / (time.perf_counter() - t0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--profile", type=int, default=0,
                    help="run only 13 pipelined steps at this B and 13 sequential ones (for a kernel trace)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("siamfc_pool_bench needs an MI355X: there is no CPU measurement")
    from mmtrack_amd import synth
    sd = synth.make_siamfc_state_dict(0)
    batches = [args.profile] if args.profile else [int(b) for b in args.batches.split(",")]
    seqs = sequences(max(batches), args.frames)
    if args.profile:
        # 13 pipelined pool steps, then 13 sequential ones: the trace holds both paths' kernels side by side
        for cfg in (Pooled(sd, seqs, args.profile, True), Sequential(sd, seqs)):
            for _ in range(13):
                cfg.step()
            cfg.drain()
            torch.cuda.synchronize()
            print(json.dumps(dict(profile=cfg.name, steps=13)))
        return
    cfgs = [Sequential(sd, seqs)]
    for B in batches:
        cfgs += [Pooled(sd, seqs, B, False), Pooled(sd, seqs, B, True)]
    for cfg in cfgs:   # warm up every shape
        for _ in range(5):
            cfg.step()
        cfg.drain()
    torch.cuda.synchronize()
    fps = {cfg.name: [] for cfg in cfgs}
    for _ in range(args.repeats):
        for cfg in cfgs:   # alternating
            fps[cfg.name].append(timed(cfg, args.seconds))
    base = float(np.median(fps["sequential"]))
    for cfg in cfgs:
        v = fps[cfg.name]
        print(json.dumps(dict(config=cfg.name, frames_per_s=round(float(np.median(v)), 1), min=round(min(v), 1),
                              max=round(max(v), 1), vs_sequential=round(float(np.median(v)) / base, 3),
                              launches_per_frame=round(13 / cfg.per_step, 3), repeats=len(v),
                              seconds_each=args.seconds)))


if __name__ == "__main__":
    main()
