"""The launches of DiMPNet.extract_backbone as a table (no device, no library: shape arithmetic only).

``layer_table(H, W, precision, stem_pool, ds_fuse)`` lists, in launch order, every conv / max-pool launch of the
two ResNet-50s to layer3 (resnet.py, Bottleneck :76-95) on an [N, 6, H, W] batch, the per-image size of every
buffer they touch and the number of max-word slots.  DiMPNet builds its launch plans from it; its FLOPs, per-layer
bytes and roofline are sums over the same rows (``row_work``).
"""
from __future__ import annotations

from typing import NamedTuple

from .synth import RESNET50_LAYERS

IMAGE = "image"   # the normalised image: as a buffer, the backbone's half; as a slot, its static range scale
OUT = "out"       # the merged layer3 map: the caller's tensor, a fresh one per forward pass (never plan-owned)


class Row(NamedTuple):
    """One launch.  Buffers are named per backbone (DiMPNet appends the backbone's index); x_slot / y_slot hold,
    per backbone of the row, the max-word slot read for the input's range and the one the epilogue accumulates
    (IMAGE: the static image scale; None: no slot -- every fp32 row, and outputs nothing reads a range of)."""
    kind: str                 # "conv" | "conv_ds": a block's conv3 with its downsample as one GEMM | "pool"
    layer: str                # "stem", "maxpool", "layerL.B.conv1/2/3", "layerL.B.downsample"
    backbones: tuple          # (0, 1): one grouped launch of the twin layers; (k,): backbone k alone
    H: int
    W: int
    Ho: int
    Wo: int
    cin: int                  # as launched: 4 for the f16x3 stem (the image padded to 4 channels)
    cout: int
    k: int
    stride: int
    pad: int
    x: str
    y: str
    x_slot: tuple
    y_slot: tuple
    relu: bool = False
    merge_max: bool = False   # max-merge into y (the aux backbone's last conv3 into the RGB layer3)
    pool: bool = False        # the stem with the 3 x 3 / stride-2 max-pool fused: Ho x Wo is the pooled map
    resid: str | None = None
    x2: str | None = None     # conv_ds: the block input the downsample reads, [x2_H, x2_W, x2_cin] at x2_stride
    x2_slot: tuple = ()
    x2_H: int = 0
    x2_W: int = 0
    x2_cin: int = 0
    x2_stride: int = 0


class Table(NamedTuple):
    rows: list
    buffers: dict   # name -> floats per image and backbone: the maximum over the rows that touch it
    nslots: int


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def layer_table(H, W, precision, stem_pool, ds_fuse, backbones=2):
    """f16x3: the twin layers of the backbones are one grouped launch, the stem writes the pooled map (stem_pool)
    and a stage's first block runs conv3 + downsample as one GEMM (ds_fuse); fp32: one launch per backbone and
    layer, in backbone order.  The last block's conv3 launches stay single in both: backbone 0 writes OUT,
    the others max-merge into it, all accumulating slot 0."""
    f16 = precision == "f16x3"
    K = tuple(range(backbones))
    rows, nslot = [], 0

    def slots(n=backbones):
        nonlocal nslot
        nslot += n if f16 else 0
        return tuple(range(nslot - n, nslot)) if f16 else (None,) * n

    def emit(layer, hw, cin, cout, k, stride, pad, x, y, xs, ys, kind="conv", split=not f16, ohw=None, **kw):
        for ks in ([(b,) for b in K] if split else [K]):
            rows.append(Row(kind, layer, ks, *hw, *(ohw or out_hw(*hw, k, stride, pad)), cin, cout, k, stride, pad,
                            x, y, tuple(xs[b] for b in ks), tuple(ys[b] for b in ks), **kw))

    none = (None,) * backbones
    out_slot, cur_s = slots(1) * backbones, slots()
    h, w = out_hw(H, W, 7, 2, 3)
    hp, wp = out_hw(h, w, 3, 2, 1)
    image_s = (IMAGE,) * backbones if f16 else none
    if f16 and stem_pool:
        emit("stem", (H, W), 4, 64, 7, 2, 3, IMAGE, "ping", image_s, cur_s, ohw=(hp, wp), relu=True, pool=True)
    else:
        emit("stem", (H, W), 4 if f16 else 3, 64, 7, 2, 3, IMAGE, "stem", image_s, cur_s, relu=True)
        # a max-pool never exceeds its input's maximum: the pooled map keeps the stem's slot
        emit("maxpool", (h, w), 64, 64, 3, 2, 1, "stem", "ping", cur_s, cur_s, kind="pool", split=True)
    h, w, cin, cur, nxt = hp, wp, 64, "ping", "pong"
    blocks = [(f"layer{li + 1}.{b}", planes, stride if b == 0 else 1, b == 0)
              for li, (planes, nb, stride) in enumerate(RESNET50_LAYERS) for b in range(nb)]
    for i, (name, planes, s, has_ds) in enumerate(blocks):
        last, cout = i == len(blocks) - 1, 4 * planes
        a_s = slots()
        emit(name + ".conv1", (h, w), cin, planes, 1, 1, 0, cur, "a", cur_s, a_s, relu=True)
        b_s = slots()
        emit(name + ".conv2", (h, w), planes, planes, 3, s, 1, "a", "b", a_s, b_s, relu=True)
        ho, wo = out_hw(h, w, 3, s, 1)
        if has_ds and f16 and ds_fuse and not last:   # relu(conv3(b) + ds(cur) + b3 + b_d)
            o_s = slots()
            emit(name + ".conv3", (ho, wo), planes, cout, 1, 1, 0, "b", nxt, b_s, o_s, kind="conv_ds", relu=True,
                 x2=cur, x2_slot=cur_s, x2_H=h, x2_W=w, x2_cin=cin, x2_stride=s)
        else:
            resid = cur
            if has_ds:   # only ever a residual operand: no max words
                emit(name + ".downsample", (h, w), cin, cout, 1, s, 0, cur, "res", cur_s, none)
                resid = "res"
            if last:
                o_s = out_slot
                for b in K:
                    rows.append(Row("conv", name + ".conv3", (b,), ho, wo, ho, wo, planes, cout, 1, 1, 0, "b", OUT,
                                    (b_s[b],), (o_s[b],), relu=True, merge_max=b > 0, resid=resid))
            else:
                o_s = slots()
                emit(name + ".conv3", (ho, wo), planes, cout, 1, 1, 0, "b", nxt, b_s, o_s, relu=True, resid=resid)
        h, w, cin, cur, nxt, cur_s = ho, wo, cout, nxt, cur, o_s
    buffers = {}
    for r in rows:
        for name, n in ((r.x, r.H * r.W * r.cin), (r.y, r.Ho * r.Wo * r.cout), (r.resid, r.Ho * r.Wo * r.cout),
                        (r.x2, r.x2_H * r.x2_W * r.x2_cin)):
            if name not in (None, OUT):
                buffers[name] = max(buffers.get(name, 0), n)
    return Table(rows, buffers, nslot)


def reference_rows(H, W, backbones=2, clf_cout=512):
    """The reference's layers as rows, backbone by backbone (a separate max-pool, an unfused downsample), then the
    clf conv (3 x 3 on the merged map): what DiMPNet.flops / layer_work / roofline_ms count."""
    rows = layer_table(H, W, "fp32", False, False, backbones).rows
    # the roofline is a float sum over this list, so its order is part of the figure: a block's downsample comes
    # after its conv3 (resnet.py:88-92), that is past the 2 * backbones launches from its own to the last conv3
    at = {id(r): i + (2 * backbones - 0.5) * r.layer.endswith(".downsample") for i, r in enumerate(rows)}
    rows = sorted(rows, key=lambda r: (r.backbones, at[id(r)]))
    h, w, c = rows[-1].Ho, rows[-1].Wo, rows[-1].cout
    return rows + [Row("conv", "clf", (0,), h, w, h, w, c, clf_cout, 3, 1, 1, OUT, "clf", (None,), (None,))]


def row_work(r):
    """(algorithmic FLOPs, minimum HBM bytes) of a row per image: 2 x MACs; the input read once, the output
    written once (and read back by a max-merge), the residual read, fp32 activations."""
    taps = r.k * r.k * r.cin + r.x2_cin
    moved = r.H * r.W * r.cin + r.x2_H * r.x2_W * r.x2_cin + \
        r.Ho * r.Wo * r.cout * (1 + (r.resid is not None) + r.merge_max)
    return (0 if r.kind == "pool" else 2 * r.Ho * r.Wo * r.cout * taps) * len(r.backbones), 4 * moved * len(r.backbones)
