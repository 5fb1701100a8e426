"""The SiamFC pool's host side, without a GPU: the three structs' layouts against the ctypes mirrors, the argument
checks of the three entry points (MMT_E_ARG before any HIP call) and the slot bookkeeping of
SiamFCPool.track_sequences (plan_slots)."""
import ctypes

import pytest

from mmtrack_amd import _lib


def test_struct_layouts_match_binding():
    lib = _lib.load()
    for which, cls in ((10, _lib.MmtSiamfcState), (11, _lib.MmtSiamfcParams), (12, _lib.MmtSiamfcResult)):
        want = [ctypes.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
        buf = (ctypes.c_size_t * 32)()
        n = lib.mmt_op_struct_layout(which, buf, 32)
        assert n == len(want), cls.__name__
        assert list(buf[:n]) == want, cls.__name__
        assert _lib.STRUCT_LAYOUTS[which] is cls
    # read as arrays by the kernels and by the host: the sizes the device code indexes with
    assert ctypes.sizeof(_lib.MmtSiamfcState) == 64 and ctypes.sizeof(_lib.MmtSiamfcResult) == 56
    assert lib.mmt_abi_version() == 10


def _params(**over):
    p = _lib.MmtSiamfcParams()
    p.scale_num, p.instance_sz, p.response_sz, p.response_up, p.total_stride = 3, 255, 17, 16, 8
    p.scale_penalty, p.scale_lr, p.window_influence, p.hann_sum = 0.9745, 0.59, 0.176, 18000.0
    for i, f in enumerate((0.96, 1.0, 1.04)):
        p.scale_factors[i] = f
    for k, v in over.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [dict(scale_num=0), dict(scale_num=9), dict(scale_num=-1), dict(instance_sz=0), dict(instance_sz=-3),
              dict(response_sz=1), dict(response_sz=0)]
D = ctypes.c_void_p(0x1000)   # a dummy non-null pointer: a call that got past the checks would report MMT_E_HIP


def test_pool_crop_rejects_bad_arguments():
    lib, ok = _lib.load(), _params()
    E = _lib.MMT_E_ARG
    assert lib.mmt_siamfc_pool_crop(None, D, 2, ctypes.byref(ok), D, D, None) == E
    assert lib.mmt_siamfc_pool_crop(D, None, 2, ctypes.byref(ok), D, D, None) == E
    assert lib.mmt_siamfc_pool_crop(D, D, 2, None, D, D, None) == E
    assert lib.mmt_siamfc_pool_crop(D, D, 2, ctypes.byref(ok), None, D, None) == E
    for n in (0, -1):
        assert lib.mmt_siamfc_pool_crop(D, D, n, ctypes.byref(ok), D, None, None) == E
    for over in BAD_PARAMS:
        assert lib.mmt_siamfc_pool_crop(D, D, 2, ctypes.byref(_params(**over)), D, None, None) == E, over


def test_pool_update_rejects_bad_arguments():
    lib, ok = _lib.load(), _params()
    E = _lib.MMT_E_ARG
    good = [D, 2, ctypes.byref(ok), D, D, D, D, None, None]
    for i in (0, 2, 3, 4, 5, 6):   # resp, params, hann1d, scratch, states, results
        a = list(good)
        a[i] = None
        assert lib.mmt_siamfc_pool_update(*a) == E, i
    for n in (0, -4):
        a = list(good)
        a[1] = n
        assert lib.mmt_siamfc_pool_update(*a) == E
    for over in BAD_PARAMS:
        a = list(good)
        a[2] = ctypes.byref(_params(**over))
        assert lib.mmt_siamfc_pool_update(*a) == E, over
        a[7] = D   # with a host record buffer as well
        assert lib.mmt_siamfc_pool_update(*a) == E, over


def test_xcorr_group_rejects_bad_arguments():
    lib = _lib.load()
    E = _lib.MMT_E_ARG
    f = ctypes.c_float

    def call(z=D, zs=9216, group=3, x=D, out=D, B=6, C=256, hz=6, wz=6, hx=22, wx=22):
        return lib.mmt_xcorr_nhwc_group(z, zs, group, x, out, B, C, hz, wz, hx, wx, f(1e-3), f(0.0), None)

    for over in (dict(z=None), dict(x=None), dict(out=None), dict(B=0), dict(B=-2), dict(group=0), dict(group=-1),
                 dict(C=0), dict(hz=0), dict(hx=5), dict(wx=5), dict(zs=-1), dict(C=512)):
        assert call(**over) == E, over


def _check_plan(lengths, capacity):
    """plan_slots' invariants: contiguous active slots, moves only from above the new count, every frame once"""
    from mmtrack_amd.siamfc import plan_slots
    steps = plan_slots(lengths, capacity)
    slots, seen, started = [], [set() for _ in lengths], []
    for st in steps:
        n = len(st["track"])
        assert 1 <= n <= capacity
        for src, dst in st["moves"]:
            assert src >= n > dst, (src, dst, n)            # only from a slot >= the new count, into a hole below
            assert slots[src] is not None
            slots[dst], slots[src] = slots[src], None
        for slot, seq in st["inits"]:
            assert slot < n and seq not in started
            assert 0 not in seen[seq]
            seen[seq].add(0)                                 # frame 0 initialises
            started.append(seq)
            slots.extend([None] * (slot + 1 - len(slots)))
            slots[slot] = seq
        assert all(s is None for s in slots[n:])
        slots = slots[:n]
        assert [s for s, _ in st["track"]] == slots          # the active slots are exactly [0, n)
        assert len(set(slots)) == n and None not in slots
        for seq, f in st["track"]:
            assert f == max(seen[seq]) + 1                   # in order, none twice
            seen[seq].add(f)
        slots = [s if max(seen[s]) + 1 < lengths[s] else None for s in slots]   # finished sequences leave holes
    assert started == list(range(len(lengths)))              # started in the order given
    for L, got in zip(lengths, seen):
        assert got == set(range(L))
    return steps


def test_slot_bookkeeping_capacity_2():
    steps = _check_plan((4, 6, 3, 5, 4), 2)
    assert [len(s["track"]) for s in steps] == [2, 2, 2, 2, 2, 2, 2, 2, 1]
    assert steps[0]["inits"] == [(0, 0), (1, 1)]
    assert steps[3] == dict(inits=[(0, 2)], moves=[], track=[(2, 1), (1, 4)])   # sequence 0's slot goes to sequence 2
    assert steps[5]["inits"] == [(0, 3), (1, 4)]                                 # 2 and 1 finish together
    assert steps[8] == dict(inits=[], moves=[], track=[(3, 4)])


def test_slot_bookkeeping_capacity_4():
    steps = _check_plan((3, 3, 3), 4)
    assert steps == [dict(inits=[(0, 0), (1, 1), (2, 2)], moves=[], track=[(0, 1), (1, 1), (2, 1)]),
                     dict(inits=[], moves=[], track=[(0, 2), (1, 2), (2, 2)])]


def test_slot_bookkeeping_moves():
    """Nothing pending and a low slot finishes: the top slot moves down, the others stay."""
    steps = _check_plan((2, 5, 3, 4), 4)
    assert steps[1]["moves"] == [(3, 0)] and steps[1]["track"] == [(3, 2), (1, 2), (2, 2)]
    _check_plan((3, 2, 2, 6, 2, 5), 3)
    assert any(s["moves"] for s in _check_plan((2, 2, 6, 3, 5), 3))   # pending runs out, then slot 0 finishes
    _check_plan((2,), 1)
    _check_plan((7, 2, 2, 2, 9), 1)
    from mmtrack_amd.siamfc import plan_slots
    with pytest.raises(ValueError):
        plan_slots((3, 1), 2)
    with pytest.raises(ValueError):
        plan_slots((3, 3), 0)
