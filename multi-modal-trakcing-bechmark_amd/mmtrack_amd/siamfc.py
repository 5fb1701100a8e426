"""SiamFC tracker on the MI355X path (RGBE/models/siamfc; the reference's folder is an empty
submodule, so this follows the published SiamFC tracker -- see oracle/siamfc.py for the restated
algorithm and DESIGN.md §8). Per frame, on the GPU:

  mmt_siamfc_crop (3-scale instance pyramid from the HBM-resident frame, cv2 INTER_LINEAR, mean-colour
  border, NHWC) -> AlexNetV1 backbone (HIP fp32-MFMA implicit-GEMM convs + max-pools, BN folded) ->
  mmt_xcorr_nhwc (HIP correlation, out_scale 1e-3) -> mmt_siamfc_response (x16 INTER_CUBIC, scale penalty, normalise, cosine window,
  argmax) -> 4 floats to the host for the box update (float64, as the reference).

GOT-10k-style tracker interface: ``init(img, box)``, ``update(img) -> box``, ``track(frames, box)``.
No CPU path: frames go to the device and every op raises without the HIP library.

``SiamFCPool`` runs many sequences per launch with the tracker state in device memory (the windows are formed
and the state advanced by the kernels; the host reads one record per sequence and frame, one frame behind);
``TrackerSiamFC`` is the sequential path and the yardstick of the pool's tests.
"""
from __future__ import annotations

import ctypes
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import rc as _rc

MMT_CONV_RELU, MMT_CONV_W4 = 1, 4   # include/mmtrack.h

CFG = dict(out_scale=0.001, exemplar_sz=127, instance_sz=255, context=0.5, scale_num=3, scale_step=1.0375,
           scale_lr=0.59, scale_penalty=0.9745, window_influence=0.176, response_sz=17, response_up=16,
           total_stride=8)


class AlexNetV1:
    """conv1 11/2 + BN + ReLU + pool3/2, conv2 5 g2 + BN + ReLU + pool, conv3 3, conv4 3 g2, conv5 3 g2 (BN eps 1e-6
    folded into the conv weights at load), on the HIP fp32-MFMA implicit-GEMM conv (``mmt_conv2d_f32_ld``: NHWC, a
    group = channel offsets into pitched rows) and ``mmt_maxpool2d_f32``.  Input: NHWC [n][H][W][3] float (what
    ``mmt_siamfc_crop_nhwc`` writes); output NHWC [n][Ho][Wo][256].  conv1's 96 output channels are zero-padded
    to 128 (the conv kernel's 64-channel tiles; the padded channels are ReLU(0) = 0 and never read by conv2)."""
    LAYERS = [("conv1", 2, 1, True, True), ("conv2", 1, 2, True, True), ("conv3", 1, 1, True, False),
              ("conv4", 1, 2, True, False), ("conv5", 1, 2, False, False)]

    def __init__(self, state_dict, device):
        self.lib = _lib.load()
        self.device = device
        self.layers = []
        cin_pitch = 3
        for li, (name, stride, groups, bn, pool) in enumerate(self.LAYERS):
            w = state_dict[f"backbone.{name}.0.weight"].double()
            b = state_dict[f"backbone.{name}.0.bias"].double()
            if bn:
                p = f"backbone.{name}.1."
                s = state_dict[p + "weight"].double() / torch.sqrt(state_dict[p + "running_var"].double() + 1e-6)
                b = (b - state_dict[p + "running_mean"].double()) * s + state_dict[p + "bias"].double()
                w = w * s.view(-1, 1, 1, 1)
            cout, cin_g, kh, kw = w.shape
            cout_g = cout // groups
            w = w.permute(0, 2, 3, 1).float()          # [Cout][kh][kw][Cin_g]
            flags = MMT_CONV_RELU if bn else 0
            if li == 0:                               # the 3-channel stem: one tap (3 values + 0) per load
                w = F.pad(w, (0, 1))
                flags |= MMT_CONV_W4
            pad_out = -cout_g % 64                    # 64-channel output tiles
            ldy = groups * (cout_g + pad_out)
            gw, gb = [], []
            for g in range(groups):
                wg = w[g * cout_g:(g + 1) * cout_g]
                bg = b[g * cout_g:(g + 1) * cout_g].float()
                if pad_out:
                    wg = torch.cat([wg, wg.new_zeros((pad_out,) + tuple(wg.shape[1:]))])
                    bg = torch.cat([bg, bg.new_zeros(pad_out)])
                gw.append(wg.contiguous().to(device))
                gb.append(bg.contiguous().to(device))
            self.layers.append(dict(w=gw, b=gb, stride=stride, groups=groups, cin_g=cin_g, ldx=cin_pitch,
                                    cout_g=cout_g + pad_out, ldy=ldy, kh=kh, kw=kw, flags=flags, pool=pool))
            cin_pitch = ldy
        self.out_channels = self.layers[-1]["ldy"]
        self._bufs = {}
        self._alloc = {}   # (H, W) -> (images allocated, their buffers)

    def reserve(self, n, H, W):
        """Allocate the activations of n images of H x W once: every call with fewer images of that size then
        runs in the first rows of these buffers (a pool at capacity serves any smaller launch)."""
        if self._alloc.get((H, W), (0, None))[0] >= n:
            return
        bufs, h, w = [], H, W
        for L in self.layers:
            h = (h - L["kh"]) // L["stride"] + 1
            w = (w - L["kw"]) // L["stride"] + 1
            y = torch.empty(n, h, w, L["ldy"], device=self.device)
            p = None
            if L["pool"]:
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
                p = torch.empty(n, h, w, L["ldy"], device=self.device)
            bufs.append((y, p))
        self._alloc[(H, W)] = (n, bufs)
        self._bufs = {k: v for k, v in self._bufs.items() if k[1:] != (H, W)}   # views of the buffers replaced

    def _buffers(self, n, H, W):
        key = (n, H, W)
        if key not in self._bufs:
            self.reserve(n, H, W)
            self._bufs[key] = [(y[:n], None if p is None else p[:n]) for y, p in self._alloc[(H, W)][1]]
        return self._bufs[key]

    def __call__(self, x, stream):
        """x: NHWC [n][H][W][3] float on the device -> NHWC features (a buffer reused by the next call of the
        same shape)."""
        n, H, W, _ = x.shape
        cur = x
        for L, (y, p) in zip(self.layers, self._buffers(n, H, W)):
            for g in range(L["groups"]):
                xo = cur.data_ptr() + 4 * g * L["cin_g"]
                yo = y.data_ptr() + 4 * g * L["cout_g"]
                _rc(self.lib.mmt_conv2d_f32_ld(xo, n, H, W, L["cin_g"], L["ldx"], L["w"][g].data_ptr(),
                                               L["b"][g].data_ptr(), L["cout_g"], L["kh"], L["kw"], L["stride"], 0,
                                               None, yo, L["ldy"], L["flags"], stream), "mmt_conv2d_f32_ld")
            H, W = y.shape[1], y.shape[2]
            cur = y
            if p is not None:
                _rc(self.lib.mmt_maxpool2d_f32(y.data_ptr(), n, H, W, L["ldy"], 3, 2, 0, p.data_ptr(), stream),
                    "mmt_maxpool2d_f32")
                H, W = p.shape[1], p.shape[2]
                cur = p
        return cur


class TrackerSiamFC:
    name = "SiamFC"
    is_deterministic = True

    def __init__(self, net_path=None, state_dict=None, device=None, **kwargs):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("TrackerSiamFC needs an MI355X (HIP device); there is no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.cfg = dict(CFG, **kwargs)
        if state_dict is None:
            state_dict = torch.load(net_path, map_location="cpu", weights_only=True)
        state_dict = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state_dict.items()}
        self.backbone = AlexNetV1(state_dict, self.device)
        c = self.cfg
        self.upscale_sz = c["response_up"] * c["response_sz"]
        h = np.hanning(self.upscale_sz)
        self.hann1d = torch.from_numpy(h).to(self.device)
        self.hann_sum = float(np.outer(h, h).sum())
        n = c["scale_num"]
        self.scale_factors = c["scale_step"] ** np.linspace(-(n // 2), n // 2, n)
        self.scratch = torch.empty(n * self.upscale_sz ** 2, device=self.device)
        self.result = torch.empty(4, device=self.device)
        self.xbuf = torch.empty(n, c["instance_sz"], c["instance_sz"], 3, device=self.device)
        self.zbuf = torch.empty(1, c["exemplar_sz"], c["exemplar_sz"], 3, device=self.device)
        self.resp = torch.empty(n, 1, c["response_sz"], c["response_sz"], device=self.device)

    def _stream(self):
        return _lib.stream(self.device)

    def _frame(self, img):
        if isinstance(img, torch.Tensor):
            t = img if img.is_cuda else img.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(img)).to(self.device, non_blocking=False)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] < 3:
            raise ValueError("frame must be H x W x C uint8 with C >= 3")
        return t.contiguous()

    def _crop(self, frame, sizes, out_sz, out):
        n = len(sizes)
        y0, x0, side = [], [], []
        for s in sizes:
            s = round(s)
            c0 = np.round(self.center - (s - 1) / 2)
            y0.append(int(np.round(c0[0])))
            x0.append(int(np.round(c0[1])))
            side.append(int(s))
        H, W, C = frame.shape
        arr = lambda v: (ctypes.c_int * len(v))(*v)
        nhwc = out.shape[-1] == 3 and out.shape[1] == out_sz
        fn = self.lib.mmt_siamfc_crop_nhwc if nhwc else self.lib.mmt_siamfc_crop
        _rc(fn(frame.data_ptr(), H, W, C, frame.stride(0), n, arr(y0), arr(x0), arr(side), arr(self.pad), out_sz,
               out.data_ptr(), self._stream()), "mmt_siamfc_crop")
        return out

    def _xcorr(self, z, x):
        """z: the exemplar's NHWC features [1][hz][wz][C] (shared by every scale), x: [n][hx][wx][C]"""
        n, hx, wx, C = x.shape
        hz, wz = z.shape[1:3]
        _rc(self.lib.mmt_xcorr_nhwc(z.data_ptr(), 0, x.data_ptr(), self.resp.data_ptr(), n, C, hz, wz, hx, wx,
                                    ctypes.c_float(self.cfg["out_scale"]), ctypes.c_float(0.0), self._stream()),
            "mmt_xcorr_nhwc")
        return self.resp

    @torch.no_grad()
    def init(self, img, box):
        c = self.cfg
        box = np.array([box[1] - 1 + (box[3] - 1) / 2, box[0] - 1 + (box[2] - 1) / 2, box[3], box[2]],
                       dtype=np.float32)
        self.center, self.target_sz = box[:2], box[2:]
        context = c["context"] * np.sum(self.target_sz)
        self.z_sz = np.sqrt(np.prod(self.target_sz + context))
        self.x_sz = self.z_sz * c["instance_sz"] / c["exemplar_sz"]
        frame = self._frame(img)
        avg = frame[..., :3].double().mean(dim=(0, 1)).cpu().numpy()
        self.avg_color = avg
        self.pad = [int(v) for v in np.clip(np.rint(avg), 0, 255)]
        z = self._crop(frame, [self.z_sz], c["exemplar_sz"], self.zbuf)
        self.kernel = self.backbone(z, self._stream()).clone()   # kept across frames (the buffer is reused)

    @torch.no_grad()
    def update(self, img):
        c = self.cfg
        frame = self._frame(img)
        x = self._crop(frame, [self.x_sz * f for f in self.scale_factors], c["instance_sz"], self.xbuf)
        resp = self._xcorr(self.kernel, self.backbone(x, self._stream()))
        _rc(self.lib.mmt_siamfc_response(resp.data_ptr(), c["scale_num"], c["response_sz"], self.upscale_sz,
                                         ctypes.c_float(c["scale_penalty"]), c["window_influence"],
                                         self.hann1d.data_ptr(), self.hann_sum, self.scratch.data_ptr(),
                                         self.result.data_ptr(), self._stream()), "mmt_siamfc_response")
        sid, ly, lx, _ = self.result.tolist()
        scale_id = int(sid)
        disp_in_response = np.array([ly, lx]) - (self.upscale_sz - 1) / 2
        disp_in_instance = disp_in_response * c["total_stride"] / c["response_up"]
        disp_in_image = disp_in_instance * self.x_sz * self.scale_factors[scale_id] / c["instance_sz"]
        self.center = self.center + disp_in_image
        scale = (1 - c["scale_lr"]) * 1.0 + c["scale_lr"] * self.scale_factors[scale_id]
        self.target_sz = self.target_sz * scale
        self.z_sz = self.z_sz * scale
        self.x_sz = self.x_sz * scale
        return np.array([self.center[1] + 1 - (self.target_sz[1] - 1) / 2,
                         self.center[0] + 1 - (self.target_sz[0] - 1) / 2,
                         self.target_sz[1], self.target_sz[0]])

    def track(self, frames, box):
        """Whole sequence: frames is a sequence of H x W x C uint8 images; returns (boxes, times)."""
        n = len(frames)
        boxes = np.zeros((n, 4))
        boxes[0] = box
        times = np.zeros(n)
        for f, img in enumerate(frames):
            begin = time.time()
            if f == 0:
                self.init(img, box)
            else:
                boxes[f, :] = self.update(img)
            times[f] = time.time() - begin
        return boxes, times


def plan_slots(lengths, capacity):
    """The slot bookkeeping of ``SiamFCPool.track_sequences`` (pure: no GPU).  ``lengths[i] >= 2`` frames of
    sequence i (frame 0 initialises, frames 1.. are tracked), ``capacity`` slots.  Returns the steps, each a dict

      inits  [(slot, seq)]  sequences initialised from their frame 0 before this step's launch
      moves  [(src, dst)]   slots re-homed first (``SiamFCPool.move``): a finished sequence's slot below the new
                            count is taken by the next pending sequence, or else by the active slot at the top
      track  [(seq, frame)] the launch: slot k tracks frame ``frame`` of sequence ``seq``, for k in [0, n)

    so the active slots are always [0, n), a move only comes from a slot >= the new count, sequences start in
    the order given and every sequence sees each of its frames exactly once."""
    if capacity < 1 or any(L < 2 for L in lengths):
        raise ValueError("plan_slots: capacity >= 1 and every sequence at least 2 frames")
    nxt = [0] * len(lengths)
    pending = list(range(len(lengths)))
    slots, steps = [], []
    while True:
        slots = [s if s is not None and nxt[s] < lengths[s] else None for s in slots]
        inits, moves = [], []
        for k in range(capacity):
            if not pending:
                break
            if k == len(slots):
                slots.append(None)
            if slots[k] is None:
                slots[k] = pending.pop(0)
                nxt[slots[k]] = 1
                inits.append((k, slots[k]))
        count = sum(s is not None for s in slots)
        for dst in range(count):
            if slots[dst] is None:
                src = max(k for k, s in enumerate(slots) if s is not None)
                moves.append((src, dst))
                slots[dst], slots[src] = slots[src], None
        slots = slots[:count]
        if not count:
            return steps
        steps.append(dict(inits=inits, moves=moves, track=[(s, nxt[s]) for s in slots]))
        for s in slots:
            nxt[s] += 1


class SiamFCPool:
    """``capacity`` SiamFC sequences with their tracker state on the device, n of them advanced per launch
    sequence: mmt_siamfc_pool_crop (windows from the states) -> one AlexNetV1 pass over n * scale_num crops ->
    mmt_xcorr_nhwc_group -> mmt_siamfc_pool_update (selection, state law, result records into pinned host
    memory).  13 launches per frame for any n, nothing read back before the next frame is launched.  Every stage
    is the sequential tracker's device code, so the boxes are ``TrackerSiamFC``'s for any n and any slot."""

    def __init__(self, state_dict=None, capacity=1, device=None, net_path=None, **cfg):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("SiamFCPool needs an MI355X (HIP device); there is no CPU path")
        if isinstance(state_dict, (str, bytes)) or hasattr(state_dict, "__fspath__"):
            net_path, state_dict = state_dict, None
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.device = dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.cfg = c = dict(CFG, **cfg)
        if state_dict is None:
            state_dict = torch.load(net_path, map_location="cpu", weights_only=True)
        state_dict = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state_dict.items()}
        self.capacity = cap = int(capacity)
        self.scale_num = S = c["scale_num"]
        if not 1 <= S <= 8:
            raise ValueError("scale_num must be 1..8")
        self.backbone = AlexNetV1(state_dict, dev)
        self.backbone.reserve(cap * S, c["instance_sz"], c["instance_sz"])
        self.upscale_sz = up = c["response_up"] * c["response_sz"]
        h = np.hanning(up)
        self.hann1d = torch.from_numpy(h).to(dev)
        self.scale_factors = c["scale_step"] ** np.linspace(-(S // 2), S // 2, S)
        self.params = self._params(c["instance_sz"], self.scale_factors, float(np.outer(h, h).sum()))
        # the exemplar crop of init(): one window of side round(z_sz) -- the init state carries z_sz as its x_sz
        self.zparams = self._params(c["exemplar_sz"], [1.0], self.params.hann_sum)
        self.sbytes, self.rbytes = ctypes.sizeof(_lib.MmtSiamfcState), ctypes.sizeof(_lib.MmtSiamfcResult)
        self.fbytes = ctypes.sizeof(_lib.MmtDimpFrame)
        self.states = torch.zeros((cap + 1) * self.sbytes, dtype=torch.uint8, device=dev)   # [cap]: init()'s scratch
        self.zbuf = torch.zeros(1, c["exemplar_sz"], c["exemplar_sz"], 3, device=dev)
        fz = self.backbone(self.zbuf, self._stream())   # its shape (the buffers of n = 1 exist from here on)
        self.exemplars = torch.zeros((cap,) + tuple(fz.shape[1:]), device=dev)
        self.xbuf = torch.empty(cap * S, c["instance_sz"], c["instance_sz"], 3, device=dev)
        self.resp = torch.empty(cap * S, c["response_sz"], c["response_sz"], device=dev)
        self.scratch = torch.empty(cap * S * up * up, device=dev)
        self.results = torch.zeros(cap * self.rbytes, dtype=torch.uint8, device=dev)
        self.init_desc = torch.zeros(self.fbytes, dtype=torch.uint8, device=dev)
        self._host_ptrs = []
        # frame descriptors and result records in mapped pinned memory the kernels read / write in place; two
        # parities, so frame k + 1 is launched before frame k's records are read
        self.desc_host = [self._host_buffer(cap * self.fbytes) for _ in range(2)]
        self.res_host = [self._host_buffer(cap * self.rbytes) for _ in range(2)]
        self._stage = {}                 # (slot, parity) -> pinned staging of a host frame
        self._launch_ev = [None, None]   # per parity: the event behind its last launch
        self._unfetched = [False, False]
        self._parity = 0

    # ------------------------------------------------------------------ plumbing
    def _params(self, out_sz, factors, hann_sum):
        c, p = self.cfg, _lib.MmtSiamfcParams()
        p.scale_num, p.instance_sz, p.response_sz = len(factors), out_sz, c["response_sz"]
        p.response_up, p.total_stride, p.scale_penalty = c["response_up"], c["total_stride"], c["scale_penalty"]
        for i, f in enumerate(factors):
            p.scale_factors[i] = float(f)
        p.scale_lr, p.window_influence, p.hann_sum = c["scale_lr"], c["window_influence"], hann_sum
        return p

    def _host_buffer(self, nbytes):
        ptr = self.lib.mmt_host_alloc(nbytes)
        if not ptr:
            raise RuntimeError("mmt_host_alloc failed")
        self._host_ptrs.append(ptr)
        return torch.frombuffer((ctypes.c_uint8 * nbytes).from_address(ptr), dtype=torch.uint8)

    def __del__(self):
        for p in getattr(self, "_host_ptrs", []):
            try:
                self.lib.mmt_host_free(p)
            except Exception:
                pass
        self._host_ptrs = []

    def _stream(self):
        return _lib.stream(self.device)

    def _state_ptr(self, slot):
        return ctypes.c_void_p(self.states.data_ptr() + slot * self.sbytes)

    def _check_slots(self, first, n):
        if n < 1 or first < 0 or first + n > self.capacity:
            raise ValueError(f"slots [{first}, {first + n}) outside the pool's {self.capacity}")

    def _device_frame(self, image, key=None):
        """A frame the kernels can index: device tensors in place, host frames through pinned staging `key`
        (None: a blocking copy) and an asynchronous copy."""
        t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] < 3:
            raise ValueError("frame must be H x W x C uint8 with C >= 3")
        if t.is_cuda:
            t = t.to(self.device)
            ok = t.stride(2) == 1 and t.stride(1) == t.shape[2] and t.stride(0) >= t.shape[1] * t.shape[2]
            return t if ok else t.contiguous()
        if key is None:
            return t.contiguous().to(self.device)
        st = self._stage.get(key)
        if st is None or st.shape != t.shape:
            st = self._stage[key] = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
        st.copy_(t)
        return st.to(self.device, non_blocking=True)

    @staticmethod
    def _describe(d, f):
        d.data, d.stride, d.H, d.W, d.C = f.data_ptr(), f.stride(0), f.shape[0], f.shape[1], f.shape[2]

    def state(self, slot):
        """The slot's device state, read back (synchronises): an ``MmtSiamfcState``."""
        self._check_slots(slot, 1)
        raw = self.states[slot * self.sbytes:(slot + 1) * self.sbytes].cpu().numpy().tobytes()
        return _lib.MmtSiamfcState.from_buffer_copy(raw)

    # ------------------------------------------------------------------ the tracker interface, per slot
    @torch.no_grad()
    def init(self, slot, img, box):
        """``TrackerSiamFC.init`` for `slot`: its host arithmetic (float32 roundings included) gives the state, the
        exemplar crop and the backbone run at n = 1 and the features go to the slot.  Stream-ordered: the border
        colour is formed and stored on the device, nothing is read back."""
        self._check_slots(slot, 1)
        c, lib, s = self.cfg, self.lib, self._stream()
        box = np.array([box[1] - 1 + (box[3] - 1) / 2, box[0] - 1 + (box[2] - 1) / 2, box[3], box[2]],
                       dtype=np.float32)
        center, target_sz = box[:2], box[2:]
        context = c["context"] * np.sum(target_sz)
        z_sz = np.sqrt(np.prod(target_sz + context))
        x_sz = z_sz * c["instance_sz"] / c["exemplar_sz"]
        frame = self._device_frame(img)
        avg = frame[..., :3].double().mean(dim=(0, 1))
        pad = torch.clamp(torch.round(avg), 0, 255).to(torch.int32)   # half to even, as np.rint
        st = _lib.MmtSiamfcState()
        st.center[0], st.center[1] = float(center[0]), float(center[1])
        st.target_sz[0], st.target_sz[1] = float(target_sz[0]), float(target_sz[1])
        st.z_sz, st.x_sz, st.frame_num = float(z_sz), float(x_sz), 0
        zst = _lib.MmtSiamfcState.from_buffer_copy(bytes(st))
        zst.x_sz = float(z_sz)
        raw = torch.frombuffer(bytearray(bytes(st) + bytes(zst)), dtype=torch.uint8).to(self.device)
        sb = self.sbytes
        self.states[slot * sb:(slot + 1) * sb].copy_(raw[:sb])
        self.states[self.capacity * sb:].copy_(raw[sb:])
        po = _lib.MmtSiamfcState.pad.offset
        for k in (slot, self.capacity):
            self.states[k * sb + po:k * sb + po + 12].view(torch.int32).copy_(pad)
        d = _lib.MmtDimpFrame()
        self._describe(d, frame)
        self.init_desc.copy_(torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8))
        _rc(lib.mmt_siamfc_pool_crop(self._state_ptr(self.capacity), ctypes.c_void_p(self.init_desc.data_ptr()), 1,
                                     ctypes.byref(self.zparams), ctypes.c_void_p(self.zbuf.data_ptr()), None, s),
            "mmt_siamfc_pool_crop")
        self.exemplars[slot].copy_(self.backbone(self.zbuf, s)[0])

    @torch.no_grad()
    def submit(self, frames, first=0):
        """Launch one frame for slots first .. first + len(frames) - 1; returns the ticket ``fetch`` takes.  One
        earlier ticket may still be unfetched."""
        n = len(frames)
        self._check_slots(first, n)
        buf = self._parity
        if self._unfetched[buf]:
            raise RuntimeError("SiamFCPool: two submitted frames are unfetched; fetch the older one first")
        if self._launch_ev[buf] is not None:
            self._launch_ev[buf].synchronize()   # this parity's descriptors / staging were read by that launch
        c, lib, s, S = self.cfg, self.lib, self._stream(), self.scale_num
        fr = [self._device_frame(f, (first + i, buf)) for i, f in enumerate(frames)]
        desc_ptr = self.desc_host[buf].data_ptr() + first * self.fbytes
        desc = (_lib.MmtDimpFrame * n).from_address(desc_ptr)
        for i, f in enumerate(fr):
            self._describe(desc[i], f)
        x = self.xbuf[:n * S]
        _rc(lib.mmt_siamfc_pool_crop(self._state_ptr(first), ctypes.c_void_p(desc_ptr), n, ctypes.byref(self.params),
                                     ctypes.c_void_p(x.data_ptr()), None, s), "mmt_siamfc_pool_crop")
        fx = self.backbone(x, s)
        z = self.exemplars[first]
        _rc(lib.mmt_xcorr_nhwc_group(ctypes.c_void_p(z.data_ptr()), z.numel(), S, ctypes.c_void_p(fx.data_ptr()),
                                     ctypes.c_void_p(self.resp.data_ptr()), n * S, fx.shape[3], z.shape[0], z.shape[1],
                                     fx.shape[1], fx.shape[2], ctypes.c_float(c["out_scale"]), ctypes.c_float(0.0), s),
            "mmt_xcorr_nhwc_group")
        _rc(lib.mmt_siamfc_pool_update(ctypes.c_void_p(self.resp.data_ptr()), n, ctypes.byref(self.params),
                                       ctypes.c_void_p(self.hann1d.data_ptr()), ctypes.c_void_p(self.scratch.data_ptr()),
                                       self._state_ptr(first), ctypes.c_void_p(self.results.data_ptr() + first * self.rbytes),
                                       ctypes.c_void_p(self.res_host[buf].data_ptr() + first * self.rbytes), s),
            "mmt_siamfc_pool_update")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._launch_ev[buf] = ev
        self._unfetched[buf] = True
        self._parity = buf ^ 1
        return ev, buf, first, n, fr   # fr: the frames stay alive until their launch has been waited for

    def fetch(self, ticket):
        """Wait for a submitted frame: (boxes [n, 4] float64 as ``TrackerSiamFC.update`` returns them, values [n],
        errs [n]; err 1: a degenerate window, that sequence kept its state)."""
        ev, buf, first, n, _ = ticket
        ev.synchronize()
        self._unfetched[buf] = False
        rec = (_lib.MmtSiamfcResult * n).from_address(self.res_host[buf].data_ptr() + first * self.rbytes)
        boxes = np.array([list(r.box) for r in rec], dtype=np.float64).reshape(n, 4)
        values = np.array([r.value for r in rec], dtype=np.float32)
        errs = np.array([r.err for r in rec], dtype=np.int32)
        self.last_selection = [(r.scale_id, r.row, r.col) for r in rec]
        return boxes, values, errs

    def update(self, frames, first=0):
        return self.fetch(self.submit(frames, first))

    @torch.no_grad()
    def move(self, src, dst):
        """Re-home slot `src` to `dst`: its state and exemplar, device to device, stream-ordered."""
        self._check_slots(src, 1)
        self._check_slots(dst, 1)
        if src == dst:
            return
        sb = self.sbytes
        self.states[dst * sb:(dst + 1) * sb].copy_(self.states[src * sb:(src + 1) * sb])
        self.exemplars[dst].copy_(self.exemplars[src])

    # ------------------------------------------------------------------ a dataset
    def track_sequences(self, seqs, on_done=None):
        """seqs: [(name, frames, init_box)] of any lengths.  Tracks them `capacity` at a time (plan_slots: active
        slots contiguous, a finished sequence's slot taken by the next pending one) with one frame of latency
        between launch and read-back.  Returns, per sequence, ``(boxes, times)`` as ``TrackerSiamFC.track``
        (times: the sequence's share of each launch's wall time); ``on_done(name, boxes, times)`` is called as
        each sequence finishes."""
        out = []
        for name, frames, box in seqs:
            boxes = np.zeros((len(frames), 4))
            if len(frames):
                boxes[0] = box
            out.append((boxes, np.zeros(len(frames))))
        live = [i for i, (_, frames, _) in enumerate(seqs) if len(frames) >= 2]
        for i in range(len(seqs)):
            if i not in live and on_done is not None:
                on_done(seqs[i][0], *out[i])
        steps = plan_slots([len(seqs[i][1]) for i in live], self.capacity)

        def finish(pend):
            ticket, track, t0 = pend
            boxes, _, _ = self.fetch(ticket)
            dt = (time.time() - t0) / len(track)
            for k, (s, f) in enumerate(track):
                i = live[s]
                out[i][0][f] = boxes[k]
                out[i][1][f] = dt
                if f == len(seqs[i][1]) - 1 and on_done is not None:
                    on_done(seqs[i][0], *out[i])

        pend = None
        for st in steps:
            t0 = time.time()
            for src, dst in st["moves"]:
                self.move(src, dst)
            for slot, s in st["inits"]:
                _, frames, box = seqs[live[s]]
                self.init(slot, frames[0], box)
            ticket = self.submit([seqs[live[s]][1][f] for s, f in st["track"]], 0)
            if pend is not None:
                finish(pend)
            pend = (ticket, st["track"], t0)
        if pend is not None:
            finish(pend)
        return out
