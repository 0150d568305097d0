"""The CLIP front end (csrc/elementwise.hip and its wiring in csrc/vit.hip) element by element against float64: ingest_kernel, im2col_kernel,
embed_ln_kernel, norm_kernel, cast_kernel, st_pool_kernel directly or through `tower.hidden_state(px, 0)`, and ln_fold_kernel / vec_mean_kernel
through `hidden_state(px, 1 | 2)` of a tower built so that their outputs matter.  Tests marked `gpu` launch kernels; the others check the
float64 references, the bounds and the negative controls and run anywhere.  u = 2^-24 is one fp32 rounding; hulp = half an ulp of the 16-bit type.

A. PREPROCESSING TABLE.  (x/255 - mean_c) / std_c has 256 x 3 distinct inputs; frames hold every byte in every channel.  The kernel computes
   v = fl(x fl(1/255)) (2 u |x/255|), fl(v - mean) (u (|x/255| + mean)), fl(. / std) (IEEE: u |q|; 2.5 ulp allowed): |q^ - q| <= 5.5 u (|x/255| +
   mean) / std, ABSOLUTE because x/255 - mean cancels near x = 123 / 117 / 104.  An output may differ from round16(q), by one ulp, only where q
   lies within W = 8 u (|x/255| + mean) / std of a rounding midpoint; everywhere else it is bitwise round16(q).  Exempt entries (counted from
   the reference alone, cap 5 % of 768 = 38): fp16 16, bf16 0, asserted below (midpoint_distance also counts the midpoint below a power of
   two, at half the spacing); the fp32 numpy emulation has no mismatch outside the window.  On the MI355X: no mismatch at all.
B. PATCH LAYOUT.  One-hot patch filters make pe[t, patch, n] = pixel (t, c, py p + i, px p + j), n = (c p + i) p + j, exactly (one non-zero product per
   sum); class embedding and positions 0, pre_layrnorm gain 1 bias 0: row (t, 1 + patch) of hidden_states[0] is the LayerNorm of that pixel vector
   (bound C with exact inputs), the CLS row is 0.  Pixels are integers in [-254, 254] (exact in both dtypes) from a hash of (t, c, y, x).
   K padding: after a 2-layer pass over inf pixels (NaN in the buffer a0 shares with fc1's output) the finite pass must repeat bitwise.
C. EMBEDDING + pre_layrnorm.  x = concat(cls, pe) + pos in float64 from the 16-bit operands; the fp32 row the kernel sees is known to
   Ex = rnd(x, Kp 2^-23 sum_k |a_k||w_k|) (accumulation as in test_gpu_gemm.py, then fl(pe + pos)).  Bound C = bounds.row_norm_bound (derivation
   there) + hulp(|ref| + E): its term rstd |gamma| Emu, Emu ~ 14 u |mu|, dominates on rows whose mean exceeds their spread.  Rows: ordinary;
   mean-dominated (class embedding + 0.625: |mu| / sigma ~ 20; position row 5 + 10: ~ 19); variance << eps (position row 8 = -pe[0, 7] + 1e-4
   noise: var ~ 1e-8); 257 rows (last workgroup: one row).  Controls (broken references the fp32 emulations must leave the bound against):
   position row n + 1, CLS from patch 0, last patch from the next frame, eps dropped, cols - 1 divisor, neighbouring channel's gain and bias.
   fp16 separates all six.  bf16's half ulp (2^-9 .. 2^-8 relative) is 4 .. 8 x the 1 / 2048 the cols - 1 divisor moves an output by, yet
   outputs within that distance of a rounding midpoint (one in eight) still leave the bound, and eps is visible on the variance << eps row:
   bf16 separates all six as well (asserted).
   The 16-frame 224 px call with n_layers = 0 runs on two lanes of 8 frames (2056 cast workgroups each, below the 4096 cap); the same call under
   the per-launch profiler runs on ONE lane (4112 workgroups: the grid-stride loop of cast_kernel is entered).  Both must be bitwise the 16
   single-frame calls; frames 0 and 15 are held to the float64 reference.
D. pgv_layernorm / pgv_rmsnorm at every instantiated width, bound C with exact inputs; rows of scale 2^-8 .. 2^6 with different offsets, a
   constant row, a row with one element 1000 x its scale; guard rows behind the last row keep their bits.  The cols - 1 control at width 256 is
   rejected in both dtypes (1 / 512 against bf16's half ulp of 2^-9 .. 2^-8).  Widths 0, 128, 1000, 1280, 4100, 8192 are refused.
E. pgv_st_pool, all four dtype pairs.  Integer inputs in [-8, 8] (bf16 inputs [-64, 64]) and the planted 256s: every partial sum is an exact
   integer, the output is fl(S fl(1 / count)) rounded to the output type.  S / count = a / b in lowest terms, b | count.  If b is a power of two
   the quotient is dyadic: when count itself is a power of two the fp32 product is exact, and an exact tie rounds to even on both sides; for the
   other counts (3, 7, 9, 17, 100: b <= 4, |a| <= 256) it is representable in bf16, no midpoint.  Otherwise the distance to a midpoint m 2^(e-1-MANT)
   of the binade [2^e, 2^(e+1)) is a non-zero multiple of 2^(e-1-MANT) / b >= 2^(e-11) / 100 (fp16 out), against an fp32 error below 3 u 2^(e+1) =
   3 x 2^(e-23): a factor >= 13.  So the output is bitwise round16(S / count) with NO exemption; the enumeration of every reachable S for every
   count used confirms it on the host, with a margin of >= 8 fp32 errors.  A host emulation of the kernel gives the same bits and loses them
   with a row group dropped, a channel chunk repeated or the frame stride of a [:, 1:] view ignored.
   Random inputs: |out - ref| <= hulp(ref) + count u mean|x|.
F. FOLDED-LAYERNORM VECTORS AND WIRING: test_folded_tower_* below (per-row error of hidden_states[1] and [2] of a tower whose out_proj / fc2 weights
   carry + 0.05, against the oracle run in the same dtype on the host), the PGV_VIT_LN_FOLD=0 path and PGV_VIT_LANES = 1 / 4 in child processes.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bounds import EPS, U32, UACC, hulp, midpoint_distance, rnd, round16, row_norm_bound
from oracle import synth
from oracle import vision as ovis

gpu = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
DTN = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SENT = 7.0                                        # guard rows
GUARD = 2
P = "vision_model."


def t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def to_dev(x64, dt):
    """float64 values that are exactly representable in dt -> device tensor of dt."""
    y = x64.to(torch.float32).to(dt)
    assert torch.equal(y.double(), x64)
    return y.to(DEV)


def violations(out, ref, bound):
    return int(((out - ref).abs() > bound).sum())


def assert_within(what, out, ref, bound):
    err = (out - ref).abs()
    ratio = float((err / bound).max())
    print(f"{what}: worst err / bound = {ratio:.3f}")
    if not bool((err <= bound).all()):
        i = np.unravel_index(int((err / bound).argmax()), err.shape)
        raise AssertionError(f"{what}: element {tuple(int(v) for v in i)}: got {float(out[i])!r}, reference {float(ref[i])!r}, bound {float(bound[i]):.3e}")


# --------------------------------------------------------------------------------------------------
# fp32 emulations of the row norm (numpy; two summation orders, both of depth <= NV + 8)
# --------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def rsqrt32(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F32)


def emu_norm_kernel_order(x, g, b, eps, rms=False):
    """The kernel's own order: lane sums over NV float4, xor butterfly over 64 lanes, FMAs where -ffp-contract=fast may form them."""
    R, n = x.shape
    NV = n // 256
    v = x.reshape(R, NV, 64, 4)

    def wave(s):
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ o]
        return s[:, :1]
    inv = F32(1.0) / F32(n)
    mean = np.zeros((R, 1), F32)
    if not rms:
        s = np.zeros((R, 64), F32)
        for i in range(NV):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        mean = wave(s) * inv
    ss = np.zeros((R, 64), F32)
    for i in range(NV):
        for e in range(4):
            d = v[:, i, :, e] - mean
            ss = fma32(d, d, ss)
    rstd = rsqrt32(wave(ss) * inv + F32(eps))
    return fma32((x - mean) * rstd, g[None], b[None])


def emu_norm_tree_order(x, g, b, eps, rms=False):
    """A balanced binary tree over the whole row (depth log2 n <= NV + 8), true division, no FMA."""
    R, n = x.shape

    def tree(a):
        m = 1 << (n - 1).bit_length()
        a = np.concatenate([a, np.zeros((R, m - n), F32)], 1)
        while a.shape[1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
        return a
    mean = np.zeros((R, 1), F32) if rms else tree(x) / F32(n)
    d = x - mean
    rstd = rsqrt32(tree(d * d) / F32(n) + F32(eps))
    return (d * rstd) * g[None] + b[None]


EMUS = [emu_norm_kernel_order, emu_norm_tree_order]


def ln64(x, g, b, eps, ddof=0):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).sum(-1, keepdim=True) / (x.shape[-1] - ddof)
    return (x - mu) * (var + eps) ** -0.5 * g + b


# ==================================================================================================
# A. preprocessing table
# ==================================================================================================
MEAN32 = [float(F32(v)) for v in ovis.CLIP_MEAN]
STD32 = [float(F32(v)) for v in ovis.CLIP_STD]
EXEMPT_CAP = int(0.05 * 768)


def byte_table():
    """uint8 [2, 16, 16, 3]: frame 0 holds every byte value once per channel (odd multipliers: permutations of 0 .. 255), frame 1 its complement."""
    idx = np.arange(256).reshape(16, 16)
    f0 = np.stack([(idx * k + o) % 256 for k, o in ((1, 0), (3, 85), (7, 170))], -1)
    return np.stack([f0, 255 - f0]).astype(np.uint8)


def preprocess_ref(frames, perm=(0, 1, 2)):
    """float64 (x/255 - mean_c) / std_c with the fp32 constants [T, 3, S, S] and the window within which the fp32 arithmetic may cross a midpoint."""
    x = t64(frames).permute(0, 3, 1, 2) / 255.0
    mean = t64([MEAN32[p] for p in perm]).view(1, 3, 1, 1)
    std = t64([STD32[p] for p in perm]).view(1, 3, 1, 1)
    return (x - mean) / std, 8 * U32 * (x.abs() + mean) / std


def check_preprocess(out, q, win, dt):
    """(elements that break the rule, exempt elements): bitwise round16(q) outside the window, within one ulp inside."""
    r = round16(q, dt)
    exempt = midpoint_distance(q, dt) <= win
    bad = torch.where(exempt, (out - r).abs() > 2 * hulp(r, dt), out != r)
    return int(bad.sum()), int(exempt.sum())


def emu_preprocess(frames):
    x = frames.astype(F32).transpose(0, 3, 1, 2) * (F32(1.0) / F32(255.0))
    mean = np.array(ovis.CLIP_MEAN, F32).reshape(1, 3, 1, 1)
    std = np.array(ovis.CLIP_STD, F32).reshape(1, 3, 1, 1)
    return t64((x - mean) / std)


@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocess_table_rule_and_controls_host(dtype):
    """Exempt entries of the 768-entry table, from the reference alone: fp16 16, bf16 0 (cap 38).  The fp32 emulation obeys the rule; a channel
    permutation of mean / std in the reference is rejected."""
    frames = byte_table()
    q, win = preprocess_ref(frames)
    out = round16(emu_preprocess(frames), dtype)
    bad, _ = check_preprocess(out, q, win, dtype)
    _, exempt = check_preprocess(out[:1], q[:1], win[:1], dtype)
    print(f"preprocess table {dtype}: {exempt} of 768 entries exempt, {bad} mismatches")
    assert bad == 0 and exempt <= EXEMPT_CAP
    assert exempt == {torch.float16: 16, torch.bfloat16: 0}[dtype]
    for perm in ((1, 2, 0), (1, 0, 2), (0, 2, 1)):
        qp, wp = preprocess_ref(frames, perm)
        assert check_preprocess(out, qp, wp, dtype)[0] > 100, perm
    assert check_preprocess(out.flip(1), q, win, dtype)[0] > 100          # channels written in the wrong order


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocess_table(ctx, dtype):
    frames = byte_table()
    q, win = preprocess_ref(frames)
    assert check_preprocess(q[:1], q[:1], win[:1], dtype)[1] <= EXEMPT_CAP
    fd = torch.from_numpy(frames).to(DEV)
    out = ctx.preprocess_u8(fd, dtype)
    assert out.shape == (2, 3, 16, 16) and out.dtype == dtype
    bad, exempt = check_preprocess(out.double().cpu(), q, win, dtype)
    print(f"pgv_preprocess_u8 {dtype}: {bad} mismatches, {exempt} exempt of {q.numel()}")
    assert bad == 0
    up = np.ascontiguousarray(frames.repeat(2, axis=1).repeat(2, axis=2))         # nearest 16 -> 32: src = floor(dst / 2)
    q2, win2 = preprocess_ref(up)
    out2 = ctx.ingest_u8(fd, 32, dtype)
    assert out2.shape == (2, 3, 32, 32) and check_preprocess(out2.double().cpu(), q2, win2, dtype)[0] == 0


# ==================================================================================================
# D. pgv_layernorm / pgv_rmsnorm
# ==================================================================================================
WIDTHS = [256, 512, 768, 1024, 2048, 4096, 5120]
ROWS = [1, 3, 4, 5, 37]
REFUSED = [0, 128, 1000, 1280, 4100, 8192]
EPS_RMS = float(F32(1e-6))


def norm_case(R, cols):
    """fp32 rows [R, cols]: row k has scale 2^(-8 + 5k mod 15) and offset scale x 1.5 x (k mod 7 - 3), so neighbours differ in both; row 1 is
    constant, row 2 carries one element 1000 x its scale."""
    g = torch.Generator().manual_seed(cols * 100 + R)
    k = torch.arange(R)
    scale = 2.0 ** (-8.0 + ((5 * k) % 15))
    off = scale * 1.5 * ((k % 7) - 3)
    x = (off[:, None] + scale[:, None] * torch.randn(R, cols, generator=g)).float()
    if R >= 3:
        x[1] = 0.7
        x[2, cols // 3] = 1000 * scale[2]
    gamma = (1 + 0.1 * torch.randn(cols, generator=g)).float()
    beta = (0.1 * torch.randn(cols, generator=g)).float()
    return x, gamma, beta


def norm_ref(x, gamma, beta, rms, dt):
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    ref, E = row_norm_bound(x, torch.zeros_like(x), gamma, torch.zeros_like(beta) if rms else beta, EPS_RMS if rms else EPS, x.shape[1] // 256, rms)
    return ref, E + hulp(ref.abs() + E, dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", WIDTHS)
def test_row_norm_bound_and_controls_host(dtype, cols):
    """Both fp32 emulations meet bound C at every width and row count; statistics taken from the neighbouring row are rejected; at width 256
    the cols - 1 divisor is rejected in both dtypes."""
    for R in ROWS:
        x, gamma, beta = norm_case(R, cols)
        for rms in (False, True):
            ref, bound = norm_ref(x, gamma, beta, rms, dtype)
            for emu in EMUS:
                out = round16(t64(emu(x.numpy(), gamma.numpy(), beta.numpy() * (0 if rms else 1), EPS_RMS if rms else EPS, rms)), dtype)
                assert violations(out, ref, bound) == 0, (R, rms, emu.__name__)
            if R >= 3:
                xd = x.double()
                mu = torch.zeros(R, 1, dtype=torch.float64) if rms else xd.mean(-1, keepdim=True)
                rstd = (((xd - mu) ** 2).mean(-1, keepdim=True) + (EPS_RMS if rms else EPS)) ** -0.5
                nb = (xd - mu.roll(1, 0) * (0 if rms else 1)) * rstd.roll(1, 0) * gamma.double() + (0 if rms else 1) * beta.double()
                assert violations(out, nb, bound) > cols // 2, (R, rms)
    if cols == 256:
        x, gamma, beta = norm_case(37, cols)
        ref, bound = norm_ref(x, gamma, beta, False, dtype)
        out = round16(t64(emu_norm_kernel_order(x.numpy(), gamma.numpy(), beta.numpy(), EPS)), dtype)
        n = violations(out, ln64(x.double(), gamma.double(), beta.double(), EPS, ddof=1), bound)
        print(f"width 256 {dtype}: the cols - 1 divisor leaves the bound at {n} of {out.numel()} elements")
        assert n > 0


def _launch_norm(ctx, x, gamma, beta, eps, dt, rms, cols, y):
    from video_llava_amd import _lib
    code, s = _lib.dtype_code(dt), _lib.stream_ptr()
    if rms:
        rc = ctx.lib.pgv_rmsnorm(ctx.handle, code, x.data_ptr(), gamma.data_ptr(), eps, y.data_ptr(), x.shape[0], cols, s)
    else:
        rc = ctx.lib.pgv_layernorm(ctx.handle, code, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, y.data_ptr(), x.shape[0], cols, s)
    _lib.check(rc, "norm")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", WIDTHS)
def test_row_norms_every_width(ctx, dtype, cols):
    worst = 0.0
    for R in ROWS:
        x, gamma, beta = norm_case(R, cols)
        xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        for rms in (False, True):
            ref, bound = norm_ref(x, gamma, beta, rms, dtype)
            y = torch.full((R + GUARD, cols), SENT, dtype=dtype, device=DEV)
            _launch_norm(ctx, xd, gd, bd, EPS_RMS if rms else EPS, dtype, rms, cols, y)
            assert bool((y[R:] == SENT).all()), f"rows behind the last were written (R={R})"
            out = y[:R].double().cpu()
            assert bool(torch.isfinite(out).all())
            worst = max(worst, float(((out - ref).abs() / bound).max()))
            assert_within(f"{'rmsnorm' if rms else 'layernorm'} {dtype} cols={cols} rows={R}", out, ref, bound)
    print(f"norm_kernel {dtype} width {cols}: worst err / bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("cols", REFUSED)
def test_row_norms_refuse_other_widths(ctx, cols):
    x = torch.zeros(4, 8192, device=DEV)
    g = torch.ones(8192, device=DEV)
    for dtype in DTYPES:
        for rms in (False, True):
            y = torch.full((4, 8192), SENT, dtype=dtype, device=DEV)
            with pytest.raises(ValueError):
                _launch_norm(ctx, x, g, g, EPS, dtype, rms, cols, y)
            torch.cuda.synchronize()
            assert bool((y == SENT).all())


@pytest.mark.parametrize("cols", REFUSED)
def test_row_norms_refuse_other_widths_host(cols):
    """launch_norm's width check runs before any device call, so the refusal is visible without a device: the entry points are handed non-null
    placeholder addresses, which a refused call never reads.  (Widths 1000 and 4100 used to launch the 768- / 4096-column kernel and return 0.)"""
    from video_llava_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for code in (_lib.PGV_F16, _lib.PGV_BF16):
        assert lib.pgv_layernorm(p, code, p, p, p, EPS, p, 4, cols, None) == _lib.PGV_EINVAL
        assert lib.pgv_rmsnorm(p, code, p, p, EPS_RMS, p, 4, cols, None) == _lib.PGV_EINVAL
        assert b"width" in lib.pgv_last_error()


# ==================================================================================================
# E. spatio-temporal pooling
# ==================================================================================================
POOL_SHAPES = [(1, 1), (3, 4), (7, 9), (8, 16), (9, 17), (100, 16)]
POOL_C = [256, 768, 1024]
PAIRS = [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)]
IN_RANGE = {torch.float16: 8, torch.bfloat16: 64}
CLS_FILL = 1000.0                                  # the row a [:, 1:] view skips (exact in both dtypes)


def pool_ref(f, n_temporal):
    """float64 [T, P, C] -> (S / count [n_temporal + P, C], sum|x| of the same sets, count per row)."""
    T, Pn, C = f.shape
    z = torch.zeros(n_temporal - T, C, dtype=torch.float64)
    ref = torch.cat([f.sum(1) / Pn, z, f.sum(0) / T])
    sabs = torch.cat([f.abs().sum(1), z, f.abs().sum(0)])
    return ref, sabs


def pool_int_input(T, Pn, C, in_dt, seed):
    g = torch.Generator().manual_seed(seed)
    X = IN_RANGE[in_dt]
    f = torch.randint(-X, X + 1, (T, Pn + 1, C), generator=g).double()
    f[:, 0] = CLS_FILL
    return f


def pool_planted_input(T, Pn, C):
    f = torch.zeros(T, Pn + 1, C, dtype=torch.float64)
    f[:, 0] = CLS_FILL
    for t in range(T):
        for p in range(Pn):
            for cb in range(C // 256):
                f[t, 1 + p, cb * 256 + (t * 31 + p * 7 + cb * 3) % 256] = 256.0
    return f


def test_pool_exact_quotients_host():
    """Every reachable integer sum S for every count the exact cases use: the fp32 emulation fl(S fl(1 / count)), rounded to the output type,
    is bitwise round16(S / count) -- no exemption is needed -- and quotients that are not exact ties stay >= 8 fp32 errors from a midpoint."""
    counts = sorted({c for tp in POOL_SHAPES for c in tp})
    for out_dt in DTYPES:
        for count in counts:
            for X in (8, 64):
                S = np.arange(-X * count, X * count + 1)
                S = np.concatenate([S, 256 * np.arange(0, count + 1)])
                q = t64(S) / count
                emu = t64(S.astype(F32) * (F32(1.0) / F32(count)))
                assert torch.equal(round16(emu, out_dt), round16(q, out_dt)), (out_dt, count, X)
                dist = midpoint_distance(q, out_dt)
                tie = (dist == 0)
                assert not bool(tie.any()) or (count & (count - 1)) == 0
                assert bool((dist[~tie] >= 8 * 3 * U32 * q.abs()[~tie]).all()), (out_dt, count, X)


def emu_pool(f, n_temporal, out_dt, defect=None):
    """st_pool_kernel in fp32 numpy on [T, P, C]: eight row groups i = grp, grp + 8, ..., combined in order, times fl(1 / count).  Defects:
    group7 = the last row group left out; chunk = the second 256-channel chunk read from the first; stride = frames read at stride P C of a
    [:, 1:] view (the caller passes the tensor WITH its skipped row for this one)."""
    x = f.numpy().astype(F32)
    if defect == "stride":
        T, P1, C = x.shape
        x = x.reshape(-1)[C:C + T * (P1 - 1) * C].reshape(T, P1 - 1, C)
    T, Pn, C = x.shape

    def mean(a):                                   # over axis 0
        acc = np.zeros((8,) + a.shape[1:], F32)
        for i in range(a.shape[0]):
            if not (defect == "group7" and i % 8 == 7):
                acc[i % 8] = acc[i % 8] + a[i]
        s = np.zeros(a.shape[1:], F32)
        for gidx in range(8):
            s = s + acc[gidx]
        return s * (F32(1.0) / F32(a.shape[0]))
    out = np.concatenate([mean(x.transpose(1, 0, 2)), np.zeros((n_temporal - T, C), F32), mean(x)])
    if defect == "chunk" and C >= 512:
        out[:, 256:512] = out[:, :256]
    return round16(t64(out), out_dt)


def test_pool_emulation_and_controls_host():
    """The fp32 emulation of the kernel gives the exact cases' expected bits; a dropped row group, a repeated channel chunk and a frame stride
    that ignores the skipped CLS row do not."""
    for (T, Pn, C) in [(9, 17, 768), (8, 16, 256), (3, 4, 1024)]:
        for in_dt, out_dt in PAIRS:
            for f in (pool_int_input(T, Pn, C, in_dt, 7), pool_planted_input(T, Pn, C)):
                want = round16(pool_ref(f[:, 1:], 12)[0], out_dt)
                assert torch.equal(emu_pool(f[:, 1:], 12, out_dt), want)
                if max(T, Pn) >= 8:
                    assert not torch.equal(emu_pool(f[:, 1:], 12, out_dt, "group7"), want)
                if C >= 512:
                    assert not torch.equal(emu_pool(f[:, 1:], 12, out_dt, "chunk"), want)
                assert not torch.equal(emu_pool(f, 12, out_dt, "stride"), want)


def _pool_exact(ctx, f, in_dt, out_dt, n_temporal, strided, what):
    T, Pn, C = f.shape[0], f.shape[1] - 1, f.shape[2]
    ref, _ = pool_ref(f[:, 1:], n_temporal)
    fd = to_dev(f, in_dt)
    view = fd[:, 1:] if strided else fd[:, 1:].contiguous()
    out = ctx.st_pool(view, n_temporal, out_dt)
    assert out.shape == (n_temporal + Pn, C) and out.dtype == out_dt
    got = out.double().cpu()
    want = round16(ref, out_dt)
    n = int((got != want).sum())
    assert n == 0, f"{what}: {n} elements differ from round16(S / count); first at {tuple(int(v) for v in (got != want).nonzero()[0])}"
    assert not bool(out[T:n_temporal].view(torch.int16).any()), f"{what}: rows [T, n_temporal) are not +0"


@gpu
@pytest.mark.parametrize("in_dt,out_dt", PAIRS)
def test_pool_exact(ctx, in_dt, out_dt):
    for (T, Pn) in POOL_SHAPES:
        for C in POOL_C:
            f = pool_int_input(T, Pn, C, in_dt, 1000 * T + 10 * Pn + C)
            for n_temporal in sorted({100, T} | ({12} if T <= 12 else set())):
                for strided in (True, False):
                    _pool_exact(ctx, f, in_dt, out_dt, n_temporal, strided, f"T={T} P={Pn} C={C} n_temporal={n_temporal} strided={strided}")
    _pool_exact(ctx, pool_planted_input(9, 17, 768), in_dt, out_dt, 12, True, "planted")
    _pool_exact(ctx, pool_planted_input(100, 16, 1024), in_dt, out_dt, 100, True, "planted, 100 frames")


@gpu
@pytest.mark.parametrize("in_dt,out_dt", PAIRS)
def test_pool_random(ctx, in_dt, out_dt):
    for (T, Pn, C) in [(9, 17, 768), (100, 16, 1024), (3, 4, 256)]:
        g = torch.Generator().manual_seed(T + Pn)
        f = round16(torch.randn(T, Pn + 1, C, generator=g, dtype=torch.float64) * 1.5, in_dt)
        ref, sabs = pool_ref(f[:, 1:], 100)
        out = ctx.st_pool(to_dev(f, in_dt)[:, 1:], 100, out_dt).double().cpu()
        assert_within(f"st_pool random {in_dt}->{out_dt} T={T} P={Pn} C={C}", out, ref, hulp(ref, out_dt) + U32 * sabs)     # count u mean|x| = u sum|x|


# ==================================================================================================
# B. patch-embedding layout          C. embedding assembly + pre_layrnorm
# ==================================================================================================
def tiny_cfg(image, layers):
    return synth.ClipCfg(hidden=1024, inter=512, layers=layers, heads=16, image=image, patch=14)


def make_tower(cfg, w, dtype):
    from helpers import make_tower as mk
    return mk(cfg, w, dtype)


def onehot_weights(cfg, seed=11):
    w = synth.make_clip_weights(cfg, seed)
    K = 3 * cfg.patch * cfg.patch
    f = np.zeros((cfg.hidden, K), F32)
    f[np.arange(K), np.arange(K)] = 1.0
    w[P + "embeddings.patch_embedding.weight"] = f.reshape(cfg.hidden, 3, cfg.patch, cfg.patch)
    w[P + "embeddings.class_embedding"] = np.zeros(cfg.hidden, F32)
    w[P + "embeddings.position_embedding.weight"] = np.zeros((cfg.tokens, cfg.hidden), F32)
    w[P + "pre_layrnorm.weight"] = np.ones(cfg.hidden, F32)
    w[P + "pre_layrnorm.bias"] = np.zeros(cfg.hidden, F32)
    return w


def pixel_pattern(T, S):
    """Integers in [-254, 254] (exact in fp16 and bf16), a hash of (t, c, y, x) no transposition of the layout preserves."""
    t, c, y, x = np.ogrid[:T, :3, :S, :S]
    return t64((t * 181 + c * 97 + y * 29 + x) % 509 - 254)


def patch_rows(px, p, defect=None):
    """[T, 3, S, S] -> [T, g g, 3 p p] in the order of CLIP's patch conv: patch = py g + px, column = (c p + i) p + j."""
    T, S = px.shape[0], px.shape[2]
    g = S // p
    if defect == "frame":
        px = px.roll(-1, 0)
    v = px.reshape(T, 3, g, p, g, p)                           # t, c, py, i, px, j
    order = {None: (0, 2, 4, 1, 3, 5), "frame": (0, 2, 4, 1, 3, 5), "ij": (0, 2, 4, 1, 5, 3), "patch": (0, 4, 2, 1, 3, 5)}[defect]
    return v.permute(*order).reshape(T, g * g, 3 * p * p)


def layout_ref(px, p, dt, defect=None):
    T = px.shape[0]
    rows = patch_rows(px, p, defect)
    x = torch.zeros(T, rows.shape[1] + 1, 1024, dtype=torch.float64)
    x[:, 1:, :rows.shape[2]] = rows
    x = x.view(-1, 1024)
    one, zero = torch.ones(1024, dtype=torch.float64), torch.zeros(1024, dtype=torch.float64)
    ref, E = row_norm_bound(x, torch.zeros_like(x), one, zero, EPS, 4)
    return x, ref, E + hulp(ref.abs() + E, dt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_patch_layout_controls_host(dtype):
    px = pixel_pattern(3, 56)
    x, ref, bound = layout_ref(px, 14, dtype)
    one, zero = np.ones(1024, F32), np.zeros(1024, F32)
    for emu in EMUS:
        out = round16(t64(emu(x.numpy().astype(F32), one, zero, EPS)), dtype)
        assert violations(out, ref, bound) == 0
        for defect in ("ij", "patch", "frame"):
            _, bad_ref, _ = layout_ref(px, 14, dtype, defect)
            assert violations(out, bad_ref, bound) > out.numel() // 4, defect


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("image,T", [(56, 3), (224, 1)])
def test_patch_layout(ctx, dtype, image, T):
    cfg = tiny_cfg(image, 1)
    tower = make_tower(cfg, onehot_weights(cfg), dtype)
    px = pixel_pattern(T, image)
    _, ref, bound = layout_ref(px, 14, dtype)
    out = tower.hidden_state(to_dev(px, dtype), 0)
    assert out.shape == (T, cfg.tokens, 1024)
    out = out.double().cpu().view(-1, 1024)
    assert not bool(out.view(T, cfg.tokens, 1024)[:, 0].any()), "CLS rows of the one-hot tower must be 0"
    assert_within(f"patch layout {dtype} {image} px", out, ref, bound)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_im2col_k_padding_is_refilled(ctx, dtype):
    cfg = tiny_cfg(56, 2)
    tower = make_tower(cfg, onehot_weights(cfg), dtype)
    px = to_dev(pixel_pattern(3, 56), dtype)
    first = tower.hidden_state(px, 0)
    poisoned = tower.hidden_state(torch.full_like(px, float("inf")), 2)
    assert bool(torch.isnan(poisoned.float()).any())            # NaN did go through fc1's output, which shares the buffer with a0
    again = tower.hidden_state(px, 0)
    assert bool(torch.isfinite(again.float()).all()) and torch.equal(again, first)


def embed_case(cfg, T, dt, seed=21):
    """Weights rounded to dt, then the planted rows (fp32 on the device): class embedding + 0.625, position row 5 + 10, position row 8 =
    -pe[0, 7] + 1e-4 noise.  Returns (weights, pixels float64, x rows float64 [T, tokens, C], Ex)."""
    rng = np.random.default_rng(seed)
    w = synth.quantize_weights(synth.make_clip_weights(cfg, seed), DTN[dt])
    px = round16(t64(rng.standard_normal((T, 3, cfg.image, cfg.image)) * 1.2), dt)
    filt = t64(w[P + "embeddings.patch_embedding.weight"]).reshape(cfg.hidden, -1)
    a = patch_rows(px, cfg.patch)
    pe = a @ filt.t()
    Kp = (a.shape[-1] + 63) // 64 * 64
    Eacc = Kp * UACC * (a.abs() @ filt.abs().t())
    w[P + "embeddings.class_embedding"] = w[P + "embeddings.class_embedding"] + F32(0.625)
    pos = w[P + "embeddings.position_embedding.weight"].copy()
    pos[5] += F32(10.0)
    pos[8] = (-pe[0, 7].numpy() + 1e-4 * rng.standard_normal(cfg.hidden)).astype(F32)
    w[P + "embeddings.position_embedding.weight"] = pos
    cls = t64(w[P + "embeddings.class_embedding"]).expand(T, 1, -1)
    x = torch.cat([cls, pe], 1) + t64(pos)
    Ex = rnd(x, torch.cat([torch.zeros_like(cls), Eacc], 1))
    return w, px, pe, x, Ex


def embed_ref(w, x, Ex, dt):
    g, b = t64(w[P + "pre_layrnorm.weight"]), t64(w[P + "pre_layrnorm.bias"])
    ref, E = row_norm_bound(x.reshape(-1, x.shape[-1]), Ex.reshape(-1, x.shape[-1]), g, b, EPS, 4)
    return ref.view(x.shape), (E + hulp(ref.abs() + E, dt)).view(x.shape)


def embed_defect(w, pe, x, defect):
    """Broken float64 references of hidden_states[0]."""
    g, b = t64(w[P + "pre_layrnorm.weight"]), t64(w[P + "pre_layrnorm.bias"])
    pos, cls = t64(w[P + "embeddings.position_embedding.weight"]), t64(w[P + "embeddings.class_embedding"])
    T = pe.shape[0]
    if defect == "pos_next":
        return ln64(x - pos + pos.roll(-1, 0), g, b, EPS)
    if defect == "cls_patch0":
        return ln64(torch.cat([pe[:, :1], pe], 1) + pos, g, b, EPS)
    if defect == "last_patch_next_frame":
        pe2 = pe.clone()
        pe2[:, -1] = pe.roll(-1, 0)[:, -1]
        return ln64(torch.cat([cls.expand(T, 1, -1), pe2], 1) + pos, g, b, EPS)
    if defect == "no_eps":
        return ln64(x, g, b, 0.0)
    if defect == "ddof":
        return ln64(x, g, b, EPS, ddof=1)
    if defect == "neighbour_affine":
        return ln64(x, g.roll(1), b.roll(1), EPS)
    raise KeyError(defect)


EMBED_DEFECTS = ["pos_next", "cls_patch0", "last_patch_next_frame", "no_eps", "ddof", "neighbour_affine"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_ln_bound_and_controls_host(dtype):
    cfg = tiny_cfg(56, 1)
    w, px, pe, x, Ex = embed_case(cfg, 3, dtype)
    ref, bound = embed_ref(w, x, Ex, dtype)
    rows = ref.view(-1, 1024)
    sig = x.std(-1)
    ratio = (x.mean(-1).abs() / sig)
    assert float(ratio[:, 0].min()) > 15 and float(ratio[:, 5].min()) > 15          # mean-dominated rows
    assert float(x[0, 8].var()) < 1e-7 and float(x[1, 8].var()) > 1e-2               # variance << eps on (0, 8) only
    pos32 = w[P + "embeddings.position_embedding.weight"]
    v32 = np.concatenate([np.broadcast_to(w[P + "embeddings.class_embedding"], (3, 1, 1024)), pe.numpy().astype(F32)], 1) + pos32[None]
    g32, b32 = w[P + "pre_layrnorm.weight"], w[P + "pre_layrnorm.bias"]
    for emu in EMUS:
        out = round16(t64(emu(v32.reshape(-1, 1024), g32, b32, EPS)), dtype)
        assert violations(out, rows, bound.view(-1, 1024)) == 0, emu.__name__
        for defect in EMBED_DEFECTS:
            n = violations(out, embed_defect(w, pe, x, defect).view(-1, 1024), bound.view(-1, 1024))
            print(f"{dtype} {emu.__name__} control {defect}: {n} elements leave the bound")
            assert n > 0, defect


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("image,T", [(56, 3), (224, 1)])
def test_embed_ln(ctx, dtype, image, T):
    cfg = tiny_cfg(image, 1)
    w, px, pe, x, Ex = embed_case(cfg, T, dtype)
    ref, bound = embed_ref(w, x, Ex, dtype)
    out = make_tower(cfg, w, dtype).hidden_state(to_dev(px, dtype), 0).double().cpu()
    assert_within(f"embed_ln {dtype} {image} px T={T}", out, ref, bound)
    if image == 56:
        for k, name in ((0, "mean-dominated CLS rows"), (5, "mean-dominated row 5"), (8, "row 8 (variance << eps in frame 0)")):
            print(f"  {name}: worst err / bound {float(((out[:, k] - ref[:, k]).abs() / bound[:, k]).max()):.3f}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_16_frames_lanes_and_cast_grid_stride(ctx, dtype):
    cfg = tiny_cfg(224, 1)
    w, px, pe, x, Ex = embed_case(cfg, 16, dtype)
    ref, bound = embed_ref(w, x, Ex, dtype)
    tower = make_tower(cfg, w, dtype)
    pd = to_dev(px, dtype)
    full = tower.hidden_state(pd, 0)                               # two lanes of 8 frames
    assert full.shape == (16, 257, 1024)
    for t in range(16):
        assert torch.equal(full[t:t + 1], tower.hidden_state(pd[t:t + 1], 0)), f"frame {t} differs from its single-frame call"
    ctx.prof_enable(True)                                          # one lane of 16 frames: 4112 > 4096 cast workgroups' worth of work
    try:
        single_lane = tower.hidden_state(pd, 0)
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert torch.equal(single_lane, full)
    got = full.double().cpu()
    for t in (0, 15):
        assert_within(f"embed_ln 16 frames {dtype} frame {t}", got[t], ref[t], bound[t])


# ==================================================================================================
# F. folded-LayerNorm load-time vectors (ln_fold_kernel, vec_mean_kernel) and the tower's wiring
# ==================================================================================================
W_OFFSET = 0.05          # added to every out_proj / fc2 weight: a sublayer then moves a row's mean by sum_k a_k W_OFFSET, a data-dependent amount
B_OFFSET = 0.25          # added to every out_proj / fc2 bias: cshift = mean(bias) is not ~ 0
BAD8 = [3, 70, 141, 200, 263, 330, 397, 500]


def folded_case(dt, T=3, seed=31):
    cfg = tiny_cfg(56, 2)
    w = synth.make_clip_weights(cfg, seed)
    for i in range(cfg.layers):
        for n in ("self_attn.out_proj", "mlp.fc2"):
            w[f"{P}encoder.layers.{i}.{n}.weight"] = w[f"{P}encoder.layers.{i}.{n}.weight"] + F32(W_OFFSET)
            w[f"{P}encoder.layers.{i}.{n}.bias"] = w[f"{P}encoder.layers.{i}.{n}.bias"] + F32(B_OFFSET)
    w = synth.quantize_weights(w, DTN[dt])
    px = round16(t64(np.random.default_rng(seed).standard_normal((T, 3, 56, 56)) * 1.2), dt)
    return cfg, w, px


def folded_hidden_states(px, w, cfg, defect=None):
    """hidden_states of the tower in float64, every LayerNorm split the way csrc/vit.hip splits it: the producer centres the new residual row at
    c = rowmean + cshift, the statistics (delta = mean(x) - c, rstd) are taken relative to c, rowmean <- rowmean + delta + cshift, and the
    consumer computes rstd (((x - c) gamma) W^T - delta colsum) + (b + W beta).  Defects: colsum_0.9 (every colsum scaled); colsum_8@<linear>@<layer>
    (eight entries of one colsum zero); gemm_no_cshift / stats_no_cshift (cshift left out on one side only)."""
    eps = cfg.eps
    x = ovis.clip_hidden_states(px, w, cfg, upto=0)[0]
    T, N, C = x.shape
    H, D = cfg.heads, C // cfg.heads
    hs = [x]
    m = x.mean(-1, keepdim=True)
    c = m
    for i in range(cfg.layers):
        def L(k):
            return ovis._t(w, f"{P}encoder.layers.{i}.{k}", torch.float64)

        def consume(x, c, ln, lin):
            g, b, Wm, bias = L(ln + ".weight"), L(ln + ".bias"), L(lin + ".weight"), L(lin + ".bias")
            colsum = Wm @ g
            if defect == "colsum_0.9":
                colsum = 0.9 * colsum
            if defect == f"colsum_8@{lin}@{i}":
                colsum = colsum.clone()
                colsum[BAD8] = 0.0
            d = x - c
            delta = d.mean(-1, keepdim=True)
            rstd = ((d * d).mean(-1, keepdim=True) - delta * delta + eps) ** -0.5
            return rstd * ((d * g) @ Wm.t() - delta * colsum) + bias + Wm @ b

        def produce(x, upd, m, bname):
            x = x + upd
            s = L(bname).mean()
            c = m + (0.0 if defect == "gemm_no_cshift" else s)
            delta = (x - c).mean(-1, keepdim=True)
            return x, c, m + delta + (0.0 if defect == "stats_no_cshift" else s)
        q, k, v = (consume(x, c, "layer_norm1", f"self_attn.{n}").view(T, N, H, D).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        o = (torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(T, N, C)
        x, c, m = produce(x, o @ L("self_attn.out_proj.weight").t() + L("self_attn.out_proj.bias"), m, "self_attn.out_proj.bias")
        h = ovis.quick_gelu(consume(x, c, "layer_norm2", "mlp.fc1"))
        x, c, m = produce(x, h @ L("mlp.fc2.weight").t() + L("mlp.fc2.bias"), m, "mlp.fc2.bias")
        hs.append(x)
    return hs


def row_rel(a, ref):
    """Relative error of every row [T * tokens]."""
    a, ref = a.double().reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return (a - ref).norm(dim=1) / ref.norm(dim=1)


def folded_yardstick(dt, T=3):
    """(cfg, weights, pixels, float64 hidden states, worst row of the oracle run in dt on the host for hidden_states[1] and [2])."""
    cfg, w, px = folded_case(dt, T)
    ref = ovis.clip_hidden_states(px, w, cfg)
    low = ovis.clip_hidden_states(px.to(dt), w, cfg)
    return cfg, w, px, ref, {k: float(row_rel(low[k], ref[k]).max()) for k in (1, 2)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_tower_controls_host(dtype):
    """The float64 model reproduces the unfolded reference (1e-12).  Measured, worst row / (1.25 x yardstick) -- the bar is 1, a control must
    reach 4: colsum x 0.9 on hidden_states[2]: fp16 64, bf16 7.2; eight zero entries of layer 1's v_proj colsum on [2]: fp16 57, bf16 6.4; in
    fp16 also on hidden_states[1]: colsum x 0.9 8.8, eight zero entries of layer 0's fc1 colsum 8.1 (bf16: 1.0 and 0.9 -- layer 0's out_proj
    moves the means too little for bf16's unit roundoff; that sublayer's colsum is visible to bf16 only through layer 1's, which the same
    kernel computes).  With W_OFFSET = 0.02 the bf16 ratios on [2] were 3.5 and 3.2, hence 0.05.
    cshift CANNOT be made visible this way: the statistics are taken relative to whatever centre the producer used, so LN(x) W^T + b = rstd (((x - c)
    gamma) W^T - (mu - c) colsum) + b' holds for ANY c, and leaving cshift out of the producer's centre or of the rowmean update (the only places
    it enters) changes nothing in exact arithmetic -- asserted here at 1e-12.  A wrong cshift costs only precision of the 16-bit operand on rows
    whose mean dominates, which tests/test_gpu_vision.py::test_folded_layernorm_mean_dominated_rows measures."""
    cfg, w, px, ref, yard = folded_yardstick(dtype)
    good = folded_hidden_states(px, w, cfg)
    assert max(float(row_rel(good[k], ref[k]).max()) for k in (1, 2)) < 1e-12
    move = float((ref[1].mean(-1) - ref[0].mean(-1)).pow(2).mean().sqrt())
    print(f"{dtype}: layer 0 moves the row means by {move:.2f} rms; yardstick worst rows {yard}")

    def ratio(defect, k):
        r = float(row_rel(folded_hidden_states(px, w, cfg, defect)[k], ref[k]).max()) / (1.25 * yard[k])
        print(f"  {defect} on hidden_states[{k}]: worst row / bar = {r:.1f}")
        return r
    assert ratio("colsum_0.9", 2) >= 4 and ratio("colsum_8@self_attn.v_proj@1", 2) >= 4
    r1, r2 = ratio("colsum_0.9", 1), ratio("colsum_8@mlp.fc1@0", 1)
    if dtype == torch.float16:
        assert r1 >= 4 and r2 >= 4
    for defect in ("gemm_no_cshift", "stats_no_cshift"):
        bad = folded_hidden_states(px, w, cfg, defect)
        assert max(float(row_rel(bad[k], ref[k]).max()) for k in (1, 2)) < 1e-12, defect


def _folded_rows(dtype):
    """Worst row of the HIP path against the float64 reference for hidden_states[1] and [2], asserted against 1.25 x the yardstick."""
    cfg, w, px, ref, yard = folded_yardstick(dtype)
    tower = make_tower(cfg, w, dtype)
    pd = to_dev(px, dtype)
    out = {}
    for k in (1, 2):
        got = tower.hidden_state(pd, k)
        assert bool(torch.isfinite(got.float()).all())
        out[k] = float(row_rel(got.cpu(), ref[k]).max())
        print(f"folded tower {dtype} hidden_states[{k}]: worst row of the HIP path {out[k]:.3e}; of the oracle in {dtype} on the host {yard[k]:.3e}")
        assert out[k] <= 1.25 * yard[k], k
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_tower_rows(ctx, dtype):
    """Per-row relative error of all 51 rows, worst row <= 1.25 x the worst row of the oracle run in the same dtype on the host.
    hidden_states[1] takes the last-layer branch of layer 0 (operand copy with gamma = 1 IS the output), [2] feeds layer 0's fc2 into layer 1's
    folded LayerNorm.  Measured on the MI355X, worst row of the path / of the yardstick: fp16 [1] 2.42e-4 / 1.05e-3, [2] 2.44e-4 / 8.84e-4; bf16 [1] 2.23e-3 /
    8.80e-3, [2] 2.01e-3 / 8.10e-3."""
    _folded_rows(dtype)


def _child(code, env):
    full = (f"import sys\nsys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            "import torch\nimport test_gpu_frontend as tf\n" + code)
    r = subprocess.run([sys.executable, "-c", full], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@gpu
def test_folded_tower_rows_unfolded_path(ctx):
    """PGV_VIT_LN_FOLD=0 (a stand-alone LayerNorm launch and a final cast; read once per process, hence a child) meets the same bar.
    Measured on the MI355X, path / yardstick: fp16 [1] 2.35e-4 / 1.05e-3, [2] 2.43e-4 / 8.84e-4; bf16 [1] 1.90e-3 / 8.80e-3, [2] 1.96e-3 / 8.10e-3."""
    out = _child("for dt in tf.DTYPES:\n    tf._folded_rows(dt)\nprint('child ok')\n", {"PGV_VIT_LN_FOLD": "0"})
    print(out)


def lanes_case(dt):
    cfg, w, _ = folded_case(dt)
    px = round16(t64(np.random.default_rng(5).standard_normal((32, 3, 56, 56)) * 1.2), dt)
    return cfg, w, px


@gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_vit_lanes_bitwise(ctx, lanes, tmp_path):
    """32 frames at 56 px: the default splits them over two lanes of 16, PGV_VIT_LANES=4 over four lanes of 8 (the threshold), =1 runs one."""
    path = str(tmp_path / "lanes.pt")
    code = ("out = {}\nfor dt in tf.DTYPES:\n    cfg, w, px = tf.lanes_case(dt)\n    out[str(dt)] = tf.make_tower(cfg, w, dt).hidden_state(tf.to_dev(px, dt), 2).cpu()\n"
            f"torch.save(out, {path!r})\nprint('child ok')\n")
    _child(code, {"PGV_VIT_LANES": str(lanes)})
    other = torch.load(path)
    for dt in DTYPES:
        cfg, w, px = lanes_case(dt)
        mine = make_tower(cfg, w, dt).hidden_state(to_dev(px, dt), 2).cpu()
        assert bool(torch.isfinite(mine.float()).all()) and torch.equal(mine, other[str(dt)]), (lanes, dt)
