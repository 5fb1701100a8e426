"""The DiMP feature net's launch table (mmtrack_amd.dimp_table) without a GPU: the launches, slots, buffer sizes,
FLOPs and bytes of ResNet-50 to layer3 x 2 (RESNET50_LAYERS = ((64, 3, 1), (128, 4, 2), (256, 6, 2))), pinned as
numbers, and the table's own consistency for every f16x3 launch variant."""
import itertools
from collections import Counter

import pytest

from mmtrack_amd.dimp_table import IMAGE, OUT, layer_table, reference_rows, row_work

SIZES = [(288, 288), (75, 61)]


@pytest.mark.parametrize("H,W", SIZES)
def test_f16x3_launch_rows(H, W):
    t = layer_table(H, W, "f16x3", True, True)
    kinds = Counter((r.kind, len(r.backbones)) for r in t.rows)
    assert len(t.rows) == 41
    assert kinds == {("conv", 2): 36, ("conv_ds", 2): 3, ("conv", 1): 2}
    assert t.nslots == 79
    # slot 0: the merged map's; the two last conv3 launches single, in backbone order, the second merging
    a, b = t.rows[-2:]
    assert (a.layer, a.backbones, a.merge_max, a.y, a.y_slot) == ("layer3.5.conv3", (0,), False, OUT, (0,))
    assert (b.layer, b.backbones, b.merge_max, b.y, b.y_slot) == ("layer3.5.conv3", (1,), True, OUT, (0,))
    assert all(r.backbones == (0, 1) and not r.merge_max for r in t.rows[:-2])
    # then the stems', then per block conv1's, conv2's and the block output's, each per backbone
    stem = t.rows[0]
    assert (stem.layer, stem.cin, stem.pool, stem.x, stem.x_slot, stem.y_slot) == ("stem", 4, True, IMAGE,
                                                                                  (IMAGE, IMAGE), (1, 2))
    assert [r.y_slot for r in t.rows[1:-2]] == [(s, s + 1) for s in range(3, 79, 2)]
    assert [r.layer for r in t.rows if r.kind == "conv_ds"] == ["layer1.0.conv3", "layer2.0.conv3", "layer3.0.conv3"]


@pytest.mark.parametrize("H,W", SIZES)
def test_fp32_launch_rows(H, W):
    t = layer_table(H, W, "fp32", True, True)
    assert len(t.rows) == 88 and t.nslots == 0
    assert Counter(r.kind for r in t.rows) == {"conv": 86, "pool": 2}
    assert all(len(r.backbones) == 1 and r.x_slot == r.y_slot == (None,) for r in t.rows)
    assert [r.backbones[0] for r in t.rows] == [0, 1] * 44   # every layer in backbone order
    assert [r.merge_max for r in t.rows] == [False] * 87 + [True]
    assert t.rows[0].cin == 3


def test_flops_and_bytes():
    for (H, W), flops, nbytes in zip(SIZES, (24_731_910_144, 1_507_094_016), (354_336_768, 21_239_016)):
        work = [row_work(r) for r in reference_rows(H, W)]
        assert len(work) == 89
        assert sum(f for f, _ in work) == flops
        assert sum(b for _, b in work) == nbytes


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_buffer_floats(precision):
    want = {"a": 38912, "b": 19456, "ping": 77824, "pong": 77824}
    if precision == "fp32":
        want.update(res=77824, stem=75392)
    want[IMAGE] = 75 * 61 * (4 if precision == "f16x3" else 3)
    assert layer_table(75, 61, precision, True, True).buffers == want


@pytest.mark.parametrize("H,W", SIZES + [(33, 50)])
@pytest.mark.parametrize("stem_pool,ds_fuse", itertools.product([True, False], repeat=2))
def test_table_is_consistent(H, W, stem_pool, ds_fuse):
    t = layer_table(H, W, "f16x3", stem_pool, ds_fuse)
    written = {(IMAGE, k): IMAGE for k in (0, 1)}   # (buffer, backbone) -> the slot its producer accumulated
    shape = {(IMAGE, k): (H, W, 4) for k in (0, 1)}
    for r in t.rows:
        for i, k in enumerate(r.backbones):
            reads = [(r.x, r.x_slot[i], (r.H, r.W, r.cin))]
            if r.x2 is not None:
                reads.append((r.x2, r.x2_slot[i], (r.x2_H, r.x2_W, r.x2_cin)))
            for name, slot, shp in reads:
                assert (name, k) in written, (r.layer, name)
                assert slot == written[name, k], (r.layer, name)   # the producer's slot, also across a max-pool
                assert shp == shape[name, k], (r.layer, name)
            if r.resid is not None:
                assert (r.resid, k) in written and shape[r.resid, k] == (r.Ho, r.Wo, r.cout), r.layer
            assert r.y not in (r.x, r.resid, r.x2), r.layer
        for i, k in enumerate(r.backbones):
            # a max-pool's output keeps the stem's slot; OUT is merged: both backbones accumulate slot 0
            written[r.y, k] = r.y_slot[i]
            shape[r.y, k] = (r.Ho, r.Wo, r.cout)
        for name in (r.x, r.y, r.resid, r.x2):
            if name not in (None, OUT):
                assert t.buffers[name] >= {r.x: r.H * r.W * r.cin, r.x2: r.x2_H * r.x2_W * r.x2_cin}.get(
                    name, r.Ho * r.Wo * r.cout)
    last = t.rows[-1]
    assert (last.Ho, last.Wo, last.cout) == ((H + 15) // 16, (W + 15) // 16, 1024)
    if (H, W) == (288, 288):
        assert (last.Ho, last.Wo) == (18, 18)
    slots = [s for r in t.rows for s in r.y_slot if isinstance(s, int)]
    assert sorted(set(slots)) == list(range(t.nslots))
    assert Counter(slots)[0] == 2 and all(n == 1 or s in (0, 1, 2) for s, n in Counter(slots).items())
