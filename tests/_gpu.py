"""What the GPU kernel tests share: layouts, the model-less engine, kept-alive device copies, operand builders and the launchers that several
tests call (a plain helper module, no pytest in it).  Importing it does not touch the device."""
import zlib

import torch
import torch.nn.functional as F

from tests import _fwd_ref, _split_ref
from tests._guards import _guarded, _guards_intact, scratch, scratch_sentinel
from videoseal_amd import native as N
from videoseal_amd.engine import Act, ConvW, HipEngine, pack_conv, rup

DEV = "cuda"
NAN = float("nan")
ISENT = 0x5A5A5A


def to_nhwc(x, ld=None):
    B, Cc, H, W = x.shape
    ld = ld or rup(Cc, 4)
    t = torch.zeros(B, H, W, ld)
    t[..., :Cc] = x.permute(0, 2, 3, 1)
    return Act(t.to(DEV).contiguous(), B, H, W, Cc, ld)


def from_nhwc(a: Act, Cc=None):
    Cc = Cc or a.C
    return a.t.view(a.B, a.H, a.W, a.ld)[..., :Cc].permute(0, 3, 1, 2).cpu()


class Eng(HipEngine):
    """engine without a model: only the kernel wrappers + workspace."""

    def __init__(self, use_split=True, arith=3):
        self.arith = arith
        self.dev = torch.device(DEV)
        self.lib = N.lib()
        self._ws = {}
        self.kernel_timers = None
        self.use_split = use_split
        self.autotune = False
        self.time_all_convs = False
        self._tile_cache = {}
        self.msg_table_conv = True
        self._ws_used = {}
        self.layer_arith = {}
        self.planes_chain = self.planes_splitk = self.msg0_planes = True
        self.planes_chain_ran = False
        self.grn_fold = self.grn_straddle = True
        self._calib = None


_KEEP = []


def dv(t):
    """device copy that stays referenced until the process ends (the C-ABI only sees raw pointers,
    so a temporary freed by Python could be recycled by the caching allocator before the kernel runs)."""
    t = t.to(DEV).contiguous()
    _KEEP.append(t)
    if len(_KEEP) > 256:
        torch.cuda.synchronize()
        del _KEEP[:128]
    return t


def rel_err(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _lib():
    return N.lib(), N.stream()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _padded(t, ld):
    """[rows, C] -> [rows, ld] with zero pad lanes"""
    out = torch.zeros(t.shape[0], ld, device=t.device)
    out[:, : t.shape[1]] = t
    return out


def r4(c):
    return (c + 3) // 4 * 4


def planes_of(h, l):
    """emulated (h, l) [rows, C] float16 -> the int16 image [2][C / 16][rows][16] of vs_to_planes"""
    rows, C = h.shape
    return torch.stack([t.view(torch.int16).view(rows, C // 16, 16).permute(1, 0, 2) for t in (h, l)], 0).contiguous().view(-1)


def rows_of(x):
    """[B, C, H, W] -> [B H W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def conv_weights(w, b, in_ld):
    wt, cp = pack_conv(dv(w), in_ld)
    return ConvW(wt, dv(b) if b is not None else None, w.shape[0], w.shape[2], w.shape[3], cp)


# ---------------------------------------------------------------------------------------------------------------- launchers shared by several tests
def wgrad_gemm_operands(case):
    rows, n, k, ldn, ldk = case
    return _split_ref.hard_dy(rows, n, 6000 + rows), _split_ref.hard_rows(rows, k, 6001 + rows)


def wgrad_gemm_launch(case):
    """(dw of vs_gemm_wgrad on the hard operands, the same from a second launch) as CPU tensors"""
    rows, n, k, ldn, ldk = case
    L, st = N.lib(), N.stream()
    dy, x = wgrad_gemm_operands(case)
    dya, xa = torch.zeros(rows, ldn, device=DEV), torch.zeros(rows, ldk, device=DEV)
    dya[:, :n], xa[:, :k] = dy.to(DEV), x.to(DEV)
    part = torch.empty(int(L.vs_gemm_wgrad_partial_floats(rows, n, k)), device=DEV)
    outs = []
    for _ in range(2):
        dw = torch.full((n, k), float("nan"), device=DEV)
        N.check(L.vs_gemm_wgrad(N.ptr(dya), ldn, n, N.ptr(xa), ldk, k, rows, N.ptr(part), N.ptr(dw), st), "vs_gemm_wgrad")
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    return outs


def attention_launch(case):
    """the kernel's output [B, H, W, heads, hd] (CPU) for one (cfg, tables?) case on the hard qkv; which kernel runs is the library's choice
    (development switch VIT_ATTN)"""
    cfg, rel = case
    B, H, W, heads, hd, win = cfg
    qkv, rh, rw = _fwd_ref.attn_inputs(cfg, rel)
    qd = qkv.to(DEV)
    rhd, rwd = (rh.to(DEV), rw.to(DEV)) if rel else (None, None)
    obuf, og = _guarded(torch.full((B, H, W, heads * hd), 9.0, device=DEV), -7.0)
    N.check(N.lib().vs_vit_attention(N.ptr(qd), B, H, W, heads, hd, win, N.ptr(rhd), N.ptr(rwd), N.ptr(og), N.stream()), "vs_vit_attention")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, -7.0), f"vs_vit_attention {case}: damaged band around the output"
    return og.cpu().view(B, H, W, heads, hd).clone()


# ---------------------------------------------------------------------------------------------------------------- ReLU decisions of the HIP forward
class _MaskedF:
    """stands in for torch.nn.functional inside oracle.videoseal_ref: relu(x) = x * mask_i with the i-th ReLU decision of the HIP forward"""

    def __init__(self, masks):
        self.masks, self.i = masks, 0

    def __getattr__(self, k):
        return getattr(F, k)

    def relu(self, x):
        m = self.masks[self.i]
        self.i += 1
        assert m.shape == x.shape, (self.i, m.shape, x.shape)
        return x * m


def hip_relu_masks(model, saved):
    """the ReLU decisions of EmbedderBackward.forward_keep in the order oracle.videoseal_ref.unet_forward calls F.relu"""
    eng = model._engine()
    L, st = eng.lib, N.stream()

    def nchw(act, t=None):
        tt = act.t if t is None else t
        return (tt.view(act.B, act.H, act.W, act.ld)[..., : act.C].permute(0, 3, 1, 2) > 0).float().cpu()

    def block(rec):
        raw1, s1 = rec["raw1"], rec["s1"]
        tmp = torch.empty_like(raw1.t)
        N.check(L.vs_scale_shift_act(N.ptr(raw1.t), raw1.rows, (raw1.C + 3) // 4 * 4, raw1.ld, N.ptr(s1["scale"]), N.ptr(s1["shift"]), N.ACT_RELU, None, 0,
                                     N.ptr(tmp), raw1.ld, st), "vs_scale_shift_act")
        return [nchw(rec["t"]), nchw(raw1, tmp)]
    masks = block(saved["inc"])
    for d in saved["downs"]:
        masks += block(d["rb"])
    for rec in saved["bott"]:
        masks += block(rec)
    for u in saved["ups"]:
        masks += [nchw(u["z"])] + block(u["rb"])
    return masks


# ---------------------------------------------------------------------------------------------------------------- scratch-size contracts
class Alloc:
    """hands out the operands of one run; `store` keeps the random master tensors so that the three runs of a case see the same values"""

    def __init__(self, mode, store):
        self.mode, self.store, self.bufs = mode, store, []

    def inp(self, t):
        t = t.cuda().contiguous()
        if self.mode == "plain":
            return t.clone()
        fill = NAN if t.is_floating_point() else ISENT
        buf, view = _guarded(t, fill)
        self.bufs.append((buf, fill))
        return view

    def rand(self, key, *shape, scale=1.0, shift=0.0, lanes=None, uniform=False):
        """random input (fixed by `key`), columns [lanes, last dim) zero: the pad lanes of an NHWC row"""
        if key not in self.store:
            g = torch.Generator(device="cuda").manual_seed(zlib.crc32(key.encode()))
            t = (torch.rand if uniform else torch.randn)(*shape, device="cuda", generator=g) * scale + shift
            if lanes is not None:
                t[..., lanes:] = 0
            self.store[key] = t
        return self.inp(self.store[key])

    def out(self, *shape, dtype=torch.float32, init=3):
        t = torch.full(shape, init, device="cuda", dtype=dtype)
        if self.mode == "plain":
            return t
        fill = -7.0 if dtype.is_floating_point else ISENT
        buf, view = _guarded(t, fill)
        self.bufs.append((buf, fill))
        return view

    def scratch(self, nelem, dtype=torch.float32):
        nelem = int(nelem)
        assert nelem > 0, "the size function answered 0 for a supported shape"
        if self.mode == "plain":
            return torch.zeros(nelem, device="cuda", dtype=dtype)
        if dtype.is_floating_point:
            fill = NAN if self.mode == "nan" else 0.0
        else:
            fill = 0xFF if self.mode == "nan" else 0          # bytes: four 0xFF are a NaN
        buf, view = scratch(nelem, dtype, fill)
        self.bufs.append((buf, scratch_sentinel(dtype)))
        return view

    def intact(self):
        return [i for i, (b, f) in enumerate(self.bufs) if not _guards_intact(b, f)]


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def _contract(case, modes=("plain", "nan", "zero")):
    """run `case(alloc)` once per mode on the same values; tests/test_gpu_scratch_contracts.py says what is asserted ("zero" only matters with a scratch)"""
    store, outs = {}, {}
    for mode in modes:
        a = Alloc(mode, store)
        res = case(a)
        torch.cuda.synchronize()
        assert not a.intact(), f"{mode}: damaged band around operand(s) {a.intact()} (in order of allocation)"
        outs[mode] = [r.clone() for r in res]
    for i, (p, n, z) in enumerate(zip(outs["plain"], outs["nan"], outs.get("zero", outs["nan"]))):
        assert torch.equal(_bits(n), _bits(z)), f"output {i} depends on what the scratch held"
        assert torch.equal(_bits(n), _bits(p)), f"output {i} differs from the unguarded call"
        assert not torch.isnan(n.double()).any(), f"output {i} holds NaN"
