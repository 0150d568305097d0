"""The MFMA GEMM (csrc/gemm.hip, gemm_w4) element by element: all ten kernel instances -- the seven public epilogues through pgv_gemm_ex with
row-major and fragment-blocked W, and the folded-LayerNorm consumer (plain, QuickGELU) and producer, which only pgv_vit_forward reached --
plus ln_stats_kernel (pgv_ln_stats) and the producer -> ln_stats -> consumer chain.  Tests marked `gpu` launch kernels; the others check the
float64 models and the bounds themselves and run anywhere.

1. EXACT tests (integer inputs).  A in [-4, 4], W in [-3, 3], integer bias and old residual: every product and every partial sum is an integer
below 2^24 (asserted on the host from sum_k |a||w| of the case), so the fp32 accumulator is exact IN ANY ORDER and the expected output does not
depend on how the kernel associates.  fp32 outputs are compared bitwise with the float64 reference; 16-bit outputs bitwise with the reference
rounded once by torch's .to(dtype).  Consumer: rstd a power of two, mean, colsum and bias integers -> rstd (acc - mean s) + b is exact.  Producer:
gnext powers of two, integer rowmean / cshift -> new residual, x16 = round16((resid - c) gnext) and EVERY (sum, sum of squares) of stats_part are
exact (sum of squares per piece < 2^24 asserted).  Padding of A and W (lda, ldw > K) is NaN; outputs sit inside NaN buffers whose guard rows,
guard columns and guard pieces must keep their bits; every launch is repeated and must give the same bits; blocked W must give the bits of
row-major W.

2. BOUND tests (real inputs), float64 reference from the 16-bit inputs, |out - ref| <= bound at EVERY element.  With u = 2^-24 (one fp32 rounding,
rnd(x, E) = E + u (|x| + E) below) the bound is assembled from the kernel's arithmetic alone:
  accumulation   |acc - exact| <= K 2^-23 S,  S = sum_k |a_k||w_k|: the products are exact, every addition rounds once, in any order; 2^-23 rather
                 than 2^-24 per addition because how the MFMA rounds its internal sums is not documented.
  BIAS / NONE    pre = rnd(acc + b).                         F32: the same, no output rounding.
  RESID          rnd(rnd(acc + b) + old).
  QuickGELU      x rcp(1 + exp2(x k)), k = -1.702f * log2(e)f: z = rnd(x k) (|k| E_x propagated), t = exp2(z) (2^E_z propagated, v_exp_f32 1 ulp =
                 2^-23), s = rnd(1 + t), r = 1 / s (E_s / (s (s - E_s)), v_rcp_f32 1 ulp), y = rnd(x r); the distance between this function with
                 the fp32 constant and the real one is added as it is.  v_exp_f32 and v_rcp_f32 are the raw instructions: a result below
                 2^-126 comes back as 0 (1 + exp2(z) > 2^126 at x < -51.6: the output is -0 where the reference is -4e-37, which bf16 can
                 hold), so each carries 2^-126 absolute on top of its ulp.
  SiLU * up      the same with k = fp32(-log2 e), then rnd(silu(g) u) with both factors' errors.
  GELU (erf)     0.5 x (1 + erff(x c)), c = fp32(2^-0.5): arg = rnd(x c), erf' = 2 pi^-0.5 exp(-arg^2) taken at the nearest point of the
                 argument's interval, erff allowed 4 ulp, s = rnd(1 + e), y = rnd((0.5 x) s).
  consumer       cc = rnd(-rstd mean), p1 = rnd(cc s_n), p2 = rnd(p1 + b'_n), p3 = rnd(rstd acc), out = rnd(p3 + p2); a contraction to FMAs only
                 removes roundings.  QuickGELU on top as above.
  producer       resid as RESID; with the centre c = fl32(rowmean + cshift) (the same single IEEE operation, reproduced in the test): d = rnd(resid - c),
                 x16 = round16(rnd(d gnext)); a piece's sum is a tree of 6 additions over 64 values: sum E_d + 6 u sum |d|; sum of squares:
                 sum (2 |d| E_d + E_d^2) + 7 u sum d^2.
  output         half an ulp of the 16-bit type at |ref| + E (subnormal spacing in fp16); nothing for fp32.
  ln_stats       s1, s2 sequential over np pieces ((np - 1) u sum |v|), delta = s1 inv (inv = fl32(1 / cols): 2 roundings), m2 likewise,
                 var = rnd(m2 - rnd(delta^2)) (the cancellation is absolute: u (m2 + delta^2) survives), v = rnd(var + eps),
                 rstd = v^-0.5 with v's interval propagated exactly and 2 ulp for rsqrtf; rowmean = rnd(rowmean + rnd(delta + cshift)).
  chain          LN(x) W2^T + b2 = rstd ((x - c) g) W2^T - rstd (mu - c) (W2 g) + (b2 + W2 beta) for ANY c, so with eps_k the error of the
                 16-bit operand (all of the producer's, plus its rounding) and e_delta, e_rstd those of the statistics,
                   out_k - out = e_rstd Z_n + rstd_k (sum_k eps_k W2[n,k] - e_delta s_n),  Z_n = (out - b'_n) / rstd,
                 to which the consumer's own arithmetic (above), the fp32 rounding of s_n and b'_n and the output rounding are added.
Nothing in a bound is taken from the kernel's output.  A failure names (row, col, tile, wave) of the worst element.  The worst err / bound per
instance and dtype is printed by every test and tabulated in DESIGN.md.

Shapes: M % 256 in {1, 127, 128, 129, 255} and M = 1 (a wave with no valid row, or a partial 128); N % 256 in {8, 64, 120, 128, 136, 192}
(a wave with no valid column, or half); K / 64 in {1, 2, 3, 4, 6, 7} (DIRECT instances: 2 = empty middle loop, 3); more tiles than CUs in
the band order (53 x 5 tiles: 265 % 8 = 1, last band of one row) and in the W-resident order (24 x 12 tiles) so that workgroups switch tiles at
every phase of the five-slot ring; N = 1024 with 65 tile rows for the DIRECT instances.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from bounds import EPS, MANT, U32, UACC, ULP1, hulp, rnd, sigmoid_mul_bound, silu_ref, swiglu_bound

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = math.nan
DTYPES = [torch.float16, torch.bfloat16]
DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}
GUARD = 3                                         # guard rows below M
NONE, BIAS, QGELU, GELU, RESID, BIAS_RESID, SWIGLU, F32, LN_BIAS, LN_QGELU, LNOUT = range(11)
EPN = ["NONE", "BIAS", "BIAS_QGELU", "BIAS_GELU", "RESID", "BIAS_RESID", "SWIGLU", "F32", "LN_BIAS", "LN_BIAS_QGELU", "BIAS_RESID_LNOUT"]
K_QGELU = float(np.float32(-1.702) * np.float32(1.4426950408889634))       # the kernel's -1.702f * 1.4426950408889634f
C_ERF = float(np.float32(0.70710678118654752))
WORST = {}                                        # (instance, dtype) -> worst err / bound seen


def quick_gelu_ref(x):
    return x / (1.0 + torch.exp(-1.702 * x))


def quick_gelu_bound(x, E):
    y, Ey = sigmoid_mul_bound(x, E, K_QGELU)
    return Ey + (y - quick_gelu_ref(x)).abs()      # the fp32 constant against the real one: part of the kernel's error


def gelu_ref(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))


def gelu_bound(x, E):
    arg = x * C_ERF
    Ea = rnd(arg, C_ERF * E)
    e = torch.erf(arg)
    near = (arg.abs() - Ea).clamp_min(0.0)
    Ee = 2.0 / math.sqrt(math.pi) * torch.exp(-near * near) * Ea + 4 * ULP1 * e.abs()
    s = 1.0 + e
    Es = rnd(s, Ee)
    h = 0.5 * x
    y = h * s
    Ey = rnd(y, h.abs() * Es + s.abs() * 0.5 * E + 0.5 * E * Es)
    return Ey + (y - gelu_ref(x)).abs()


def consumer_bound(acc, Eacc, mean, rstd, s, b):
    """rstd (acc - mean s) + b as a d + (c s + b) with c = -rstd mean (mean, rstd [M,1]; s, b [1,N] exact fp32 inputs)."""
    cc = -rstd * mean
    Ecc = U32 * cc.abs()
    p1 = cc * s
    E1 = rnd(p1, s.abs() * Ecc)
    p2 = p1 + b
    E2 = rnd(p2, E1)
    p3 = rstd * acc
    E3 = rnd(p3, rstd * Eacc)
    out = p3 + p2
    return out, rnd(out, E3 + E2)


def producer_bound(rnew, Er, c, gn, dt, NP):
    """Centre, 16-bit operand and partial statistics of the producer from the new residual rnew (known to Er) and the exact centre c [M,1]."""
    d = rnew - c
    Ed = rnd(d, Er)
    x = d * gn
    Ex = rnd(x, gn.abs() * Ed)
    Ex16 = Ex + hulp(x.abs() + Ex, dt)
    M = d.shape[0]
    dp, Ep = d.view(M, NP, 64), Ed.view(M, NP, 64)
    mag = dp.abs() + Ep
    t1, E1 = dp.sum(-1), Ep.sum(-1) + 6 * U32 * mag.sum(-1)
    t2, E2 = (dp * dp).sum(-1), (2 * dp.abs() * Ep + Ep * Ep).sum(-1) + 7 * U32 * (mag * mag).sum(-1)
    return x, Ex16, t1, E1, t2, E2                 # statistics as [M, NP]


def ln_stats_bound(t1, E1, t2, E2, cols, eps):
    """ln_stats_kernel on partial sums [M, NP] known to E1, E2: (delta, E), (rstd, E)."""
    NP = t1.shape[1]
    s1, s2 = t1.sum(1), t2.sum(1)
    Es1 = E1.sum(1) + (NP - 1) * U32 * (t1.abs() + E1).sum(1)
    Es2 = E2.sum(1) + (NP - 1) * U32 * (t2.abs() + E2).sum(1)
    delta, m2 = s1 / cols, s2 / cols
    Edl = Es1 / cols + 2 * U32 * (delta.abs() + Es1 / cols)
    Em2 = Es2 / cols + 2 * U32 * (m2.abs() + Es2 / cols)
    sq = delta * delta
    Esq = rnd(sq, 2 * delta.abs() * Edl + Edl * Edl)
    var = (m2 - sq).clamp_min(0.0)
    Evar = rnd(var, Em2 + Esq)
    v = var + eps
    Ev = rnd(v, Evar)
    rstd = v ** -0.5
    lo = (v - Ev).clamp_min(1e-300)
    Er = lo ** -0.5 - rstd
    Er = Er + 2 * ULP1 * (rstd + Er)
    return delta, Edl, rstd, Er


def dropped_slice(a, w, row0, col0, k0):
    """The float64 product with one 16-deep k slice of one 32x32 block left out (negative control of the bounds)."""
    acc = a @ w.t()
    acc[row0:row0 + 32, col0:col0 + 32] -= a[row0:row0 + 32, k0:k0 + 16] @ w[col0:col0 + 32, k0:k0 + 16].t()
    return acc


# --------------------------------------------------------------------------------------------------
# the folded LayerNorm in float64
# --------------------------------------------------------------------------------------------------
def folded_ln_model(r, gamma, beta, W2, b2, c, eps, defect=None):
    """LayerNorm(r) W2^T + b2 computed the way the three kernels split it, in float64, with the row centre c [M,1] (any value).  `defect`:
    no_centre = the operand is not centred although the statistics are; piece_order = the piece-major partial array read row-major;
    mean_for_delta = the consumer is handed the row mean in place of mean - c."""
    M, C = r.shape
    NP = C // 64
    d = r - c
    x = (r if defect == "no_centre" else d) * gamma
    part = torch.stack([d.view(M, NP, 64).sum(-1), (d * d).view(M, NP, 64).sum(-1)], -1).transpose(0, 1).contiguous()      # [NP][M][2]
    if defect == "piece_order":
        part = part.reshape(M, NP, 2).transpose(0, 1)
    s1, s2 = part[..., 0].sum(0), part[..., 1].sum(0)
    delta = s1 / C
    rstd = (s2 / C - delta * delta + eps) ** -0.5
    if defect == "mean_for_delta":
        delta = delta + c[:, 0]
    colsum = W2 @ gamma
    b2f = b2 + W2 @ beta
    return rstd[:, None] * (x @ W2.t() - delta[:, None] * colsum) + b2f


def layer_norm_linear(r, gamma, beta, W2, b2, eps):
    return torch.nn.functional.layer_norm(r, (r.shape[1],), gamma, beta, eps) @ W2.t() + b2


# --------------------------------------------------------------------------------------------------
# host-only tests of the models and bounds
# --------------------------------------------------------------------------------------------------
def _ln_case(M, C, N, seed, ratio=20.0):
    g = torch.Generator().manual_seed(seed)
    sig = 0.5 + torch.rand(M, 1, generator=g, dtype=torch.float64)
    mu = sig * torch.linspace(-ratio, ratio, M, dtype=torch.float64)[:, None]
    r = mu + sig * torch.randn(M, C, generator=g, dtype=torch.float64)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    W2 = 0.05 * torch.randn(N, C, generator=g, dtype=torch.float64)
    b2 = torch.randn(N, generator=g, dtype=torch.float64)
    return r, gamma, beta, W2, b2, mu


def test_centred_identity_reproduces_layer_norm_for_any_centre():
    """Host only.  The float64 model of the three-kernel split equals layer_norm followed by the Linear to 1e-12 whatever the centre (0, the
    exact mean, a stale mean, a far-off value), on rows with |mean| / sigma up to 20; each broken model misses by many orders more."""
    r, gamma, beta, W2, b2, mu = _ln_case(37, 320, 72, 5)
    want = layer_norm_linear(r, gamma, beta, W2, b2, 1e-5)
    scale = want.abs().max()
    for c in (torch.zeros(37, 1, dtype=torch.float64), r.mean(1, keepdim=True), mu + 0.3, mu * 0.5 - 7.0):
        got = folded_ln_model(r, gamma, beta, W2, b2, c, 1e-5)
        assert float((got - want).abs().max() / scale) < 1e-12
    c = mu + 0.3
    for defect in ("no_centre", "piece_order", "mean_for_delta"):
        bad = folded_ln_model(r, gamma, beta, W2, b2, c, 1e-5, defect)
        assert float((bad - want).abs().max() / scale) > 1e-3, defect


def test_bounds_reject_a_dropped_k_slice_and_a_row_added_twice():
    """Host only.  The per-element bound of every epilogue family sits far below what one missing 16-deep k slice of one 32x32 block, or one row
    taken through the read-modify-write twice, does to an output -- and above the error of honest fp32 arithmetic."""
    g = torch.Generator().manual_seed(11)
    for dt in DTYPES:
        M, N, K = 96, 128, 448
        a = torch.randn(M, K, generator=g).to(dt).double()
        w = (0.08 * torch.randn(N, K, generator=g)).to(dt).double()
        b = torch.randn(N, generator=g).double()
        old = torch.randn(M, N, generator=g).double()
        acc, S = a @ w.t(), a.abs() @ w.abs().t()
        Eacc = K * UACC * S
        pre, Epre = acc + b, rnd(acc + b, Eacc)
        bad = dropped_slice(a, w, 32, 64, 416) + b
        blk = (slice(32, 64), slice(64, 96))
        honest32 = (a.float() @ w.float().t() + b.float()).double()
        assert ((honest32 - pre).abs() <= Epre).all()
        b16 = Epre + hulp(pre.abs() + Epre, dt)
        assert ((honest32.to(dt).double() - pre).abs() <= b16).all()
        # 16-bit output: some element of the block leaves the bound; fp32 outputs and the residual: (nearly) every element does
        assert (~((bad.to(dt).double() - pre).abs() <= b16))[blk].any()
        assert (~((bad - pre).abs() <= Epre))[blk].double().mean() > 0.9
        rn, Ern = old + pre, rnd(old + pre, Epre)
        twice = rn.clone()
        twice[77] += pre[77]
        assert (~((twice - rn).abs() <= Ern))[77].double().mean() > 0.9
        for ref, Eb, f in ((quick_gelu_ref(pre), quick_gelu_bound(pre, Epre), quick_gelu_ref), (gelu_ref(pre), gelu_bound(pre, Epre), gelu_ref)):
            Eb = Eb + hulp(ref.abs() + Eb, dt)
            assert ((f(honest32).float().to(dt).double() - ref).abs() <= Eb).all()
            assert (~((f(bad).to(dt).double() - ref).abs() <= Eb))[blk].any()
        # statistics of the producer: one wrong element moves the piece's sums out of their bound
        NP = N // 64
        c = rn.mean(1, keepdim=True)
        _, _, t1, E1, t2, E2 = producer_bound(rn, Ern, c, torch.ones(N, dtype=torch.float64), dt, NP)
        _, _, u1, _, u2, _ = producer_bound(twice, Ern, c, torch.ones(N, dtype=torch.float64), dt, NP)
        assert ((u1 - t1).abs() > E1)[77].all() and ((u2 - t2).abs() > E2)[77].all()


def test_ln_stats_bound_holds_for_fp32_arithmetic_and_rejects_a_wrong_divisor():
    """Host only.  The ln_stats bound covers a plain fp32 evaluation (sequential sums, E[x^2] - delta^2, rsqrt) on mean-dominated and
    zero-variance rows, and rejects statistics computed with cols - 1 in place of cols."""
    t1, t2, _ = _stats_case(64, 16, "cpu", 3)
    cols = 16 * 64
    delta, Edl, rstd, Er = ln_stats_bound(t1.double(), torch.zeros_like(t1, dtype=torch.float64), t2.double(), torch.zeros_like(t2, dtype=torch.float64), cols, EPS)
    s1, s2 = torch.zeros(64), torch.zeros(64)
    for i in range(16):
        s1, s2 = s1 + t1[:, i], s2 + t2[:, i]
    inv = torch.tensor(1.0 / cols, dtype=torch.float32)
    d32 = s1 * inv
    r32 = torch.rsqrt((s2 * inv - d32 * d32).clamp_min(0) + torch.tensor(EPS, dtype=torch.float32))
    assert ((d32.double() - delta).abs() <= Edl).all() and ((r32.double() - rstd).abs() <= Er).all()
    dbad = s1.double() / (cols - 1)
    assert ((dbad - delta).abs() > Edl)[s1 != 0].all()


def _stats_case(M, NP, dev, seed):
    """Partial sums [M, NP] (fp32, exactly what the kernel reads) of rows with delta / sigma from 0 to 20, two rows of variance 0 and a zero row."""
    g = torch.Generator(device=dev).manual_seed(seed)
    C = NP * 64
    sig = 0.25 + torch.rand(M, 1, generator=g, device=dev, dtype=torch.float64)
    dl = sig * torch.linspace(-20, 20, M, device=dev, dtype=torch.float64)[:, None]
    d = dl + sig * torch.randn(M, C, generator=g, device=dev, dtype=torch.float64)
    d[1] = 0.25
    d[M // 2] = -3.0
    d[2] = 0.0
    t1 = d.view(M, NP, 64).sum(-1).float()
    t2 = (d * d).view(M, NP, 64).sum(-1).float()
    return t1, t2, d


# --------------------------------------------------------------------------------------------------
# launch helpers
# --------------------------------------------------------------------------------------------------
def bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def ptr(t):
    return t.data_ptr() if t is not None else None


def gemm_ex(ctx, dt, epi, A, W, C, M, N, K, bias=None, blocked=False, ldw=None, rowstat=None, colsum=None, gnext=None, x16=None, stats=None,
            rowmean=None, cshift=None, lda=None, ldc=None, ldx16=None, ok=True):
    from video_llava_amd import _lib
    d = _lib.GemmDesc()
    d.d_A, d.lda = ptr(A), A.stride(0) if lda is None else lda
    d.d_W, d.ldw, d.w_blocked = ptr(W), (K if blocked else W.stride(0)) if ldw is None else ldw, 1 if blocked else 0
    d.d_bias, d.d_C, d.ldc = ptr(bias), ptr(C), C.stride(0) if ldc is None else ldc
    d.M, d.N, d.K, d.epi = M, N, K, epi
    d.d_rowstat, d.d_colsum, d.d_gnext, d.d_x16 = ptr(rowstat), ptr(colsum), ptr(gnext), ptr(x16)
    d.ldx16 = (x16.stride(0) if x16 is not None else 0) if ldx16 is None else ldx16
    d.d_stats_part, d.d_rowmean, d.d_cshift = ptr(stats), ptr(rowmean), ptr(cshift)
    rc = ctx.lib.pgv_gemm_ex(ctx.handle, _lib.dtype_code(dt), ctypes.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    if ok:
        _lib.check(rc, "pgv_gemm_ex")
    return rc


def pack_blocked(ctx, w):
    from video_llava_amd import _lib
    N, K = w.shape
    src = w.contiguous()
    dst = torch.zeros((N + 15) // 16 * 16 * K, dtype=w.dtype, device=w.device)
    _lib.check(ctx.lib.pgv_pack_blocked(ctx.handle, _lib.dtype_code(w.dtype), src.data_ptr(), N, K, dst.data_ptr(), _lib.stream_ptr()), "pgv_pack_blocked")
    torch.cuda.synchronize()
    return dst


def padded(x, pad):
    """x [R, K] inside a NaN buffer of row stride K + pad."""
    full = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=x.dtype, device=x.device)
    full[:, :x.shape[1]] = x
    return full[:, :x.shape[1]]


class Embedded:
    """An [M, N] output inside a NaN buffer with GUARD rows below, `gcols` columns to the right and `offset` elements in front."""

    def __init__(self, M, N, dt, init=None, gcols=4, offset=0, rows_extra=GUARD):
        self.M, self.N, self.ld = M, N, N + gcols
        self.buf = torch.full(((M + rows_extra) * self.ld + offset,), NAN, dtype=dt, device=DEV)
        self.full = self.buf[offset:].view(M + rows_extra, self.ld)
        self.view = self.full[:M, :N]
        if init is not None:
            self.view.copy_(init)
        self.before = self.buf.clone()

    def guards_untouched(self):
        after = self.buf.clone()
        off = self.buf.numel() - self.full.numel()
        after[off:].view_as(self.full)[:self.M, :self.N] = self.before[off:].view_as(self.full)[:self.M, :self.N]
        return torch.equal(bits(after), bits(self.before))


def where(r, c):
    return f"row {r} col {c} tile ({r // 256}, {c // 256}) wave {((r % 256) // 128) * 2 + (c % 256) // 128}"


def assert_bits(got, want, what):
    """Bitwise equality of two [M, N] tensors of one dtype (+0 and -0 differ, every NaN differs from a number)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ne = bits(got) != bits(want)
    if ne.any():
        r, c = [int(v) for v in ne.nonzero()[0]]
        rows = ne.any(1).sum()
        raise AssertionError(f"{what}: {int(ne.sum())} elements in {int(rows)} rows differ; first at {where(r, c)}: got {float(got[r, c])!r} want {float(want[r, c])!r}")


def assert_bound(got, ref, bound, what, key):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = float(ratio.max())
    i = int(ratio.argmax())
    r, c = divmod(i, ratio.shape[1]) if ratio.dim() == 2 else (i, 0)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"\n[gemm] {what}: worst err/bound {worst:.3f} at {where(r, c)}; so far {({f'{k[0]}/{k[1]}': round(v, 3) for k, v in WORST.items()})}")
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside the bound; worst at {where(r, c)}: got {float(got.reshape(ratio.shape).flatten()[i])!r} "
                           f"ref {float(ref.flatten()[i])!r} bound {float(bound.flatten()[i]):.3e}")


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g, device=DEV).double()


def distinct(x):
    return torch.unique(x, dim=0).shape[0] == x.shape[0]


@functools.lru_cache(maxsize=4)
def int_case(M, N, K):
    g = gen(M * 31 + N * 7 + K)
    a, w = ints((M, K), 4, g), ints((N, K), 3, g)
    assert distinct(a) and distinct(w), "integer case with repeated rows of A or W (output rows / columns): change the seed"
    b, old = ints((N,), 8, g), ints((M, N), 64, g)
    acc = a @ w.t()
    S = float((a.abs() @ w.abs().t()).max())
    assert S + 8 + 64 < 2 ** 24, "a partial sum may leave fp32's integer range"
    return a, w, b, old, acc


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# --------------------------------------------------------------------------------------------------
# 1. exact tests
# --------------------------------------------------------------------------------------------------
def run_exact_public(ctx, dt, M, N, K, epis, what):
    a, w, b, old, acc = int_case(M, N, K)
    A, W = padded(a.to(dt), 8), padded(w.to(dt), 16)
    Wb = pack_blocked(ctx, w.to(dt)) if N % 16 == 0 else None
    b32 = b.float()
    for epi in epis:
        out32 = epi in (RESID, BIAS_RESID, F32)
        odt = torch.float32 if out32 else dt
        want = {NONE: lambda: acc, BIAS: lambda: acc + b, F32: lambda: acc + b, RESID: lambda: old + acc, BIAS_RESID: lambda: old + acc + b}[epi]().to(odt)
        init = old.float() if epi in (RESID, BIAS_RESID) else None
        first = None
        for layout in ("row", "row", "blk") if Wb is not None else ("row", "row"):
            # 16-bit outputs start 8 bytes into the allocation (8- but not 16-byte aligned) with a row pitch of N + 4 elements
            o = Embedded(M, N, odt, init=init, gcols=4, offset=0 if out32 else 4)
            assert out32 or o.view.data_ptr() % 16 == 8
            gemm_ex(ctx, dt, epi, A, Wb if layout == "blk" else W, o.view, M, N, K, bias=None if epi in (NONE, RESID) else b32, blocked=layout == "blk")
            tag = f"{what} {EPN[epi]} {layout}"
            assert o.guards_untouched(), f"{tag}: guard rows / columns / leading bytes of the output buffer were written"
            assert torch.isfinite(o.view.float()).all(), f"{tag}: non-finite output (padding read, or an element not written)"
            assert_bits(o.view, want, tag)
            if first is None:
                first = o.view.clone()
            else:
                assert_bits(o.view, first, f"{tag} against the first launch")


RAGGED = [(1, 264, 64), (257, 64, 128), (383, 376, 192), (128, 128, 256), (385, 392, 384), (511, 448, 448), (300, 528, 128)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K", RAGGED, ids=[f"{m}x{n}x{k}" for m, n, k in RAGGED])
def test_exact_public_epilogues_ragged(ctx, dt, M, N, K):
    """M = 1 and last row tiles of 1 / 127 / 128 / 129 / 255 rows, N % 256 in {8, 64, 120, 128, 136, 192} and blocked N = 528, K / 64 in
    {1, 2, 3, 4, 6, 7}, lda / ldw / ldc beyond the logical sizes with NaN in between, an 8-byte aligned 16-bit C: bitwise."""
    run_exact_public(ctx, dt, M, N, K, (NONE, BIAS, F32, RESID, BIAS_RESID), f"exact {M}x{N}x{K} {DTN[dt]}")


BAND = (52 * 256 + 129, 1168)                      # 53 x 5 tiles, band order: 265 % 8 = 1, last band of one tile row
WRES = (23 * 256 + 255, 3008)                      # 24 x 12 tiles, W-resident order
WALK = [(*s, 64 * nk) for s in (BAND, WRES) for nk in (1, 2, 3, 4, 6, 7)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K", WALK, ids=[f"{'band' if n == BAND[1] else 'wres'}-nk{k // 64}" for m, n, k in WALK])
def test_exact_tile_walk(ctx, dt, M, N, K):
    """More tiles than CUs in both tile orders, so that workgroups walk from one tile to the next at ring phases 2 nk mod 5 for
    nk in {1, 2, 3, 4, 6, 7}; ragged last row tile and last column tile; 16-bit, fp32 read-modify-write and blocked W: bitwise."""
    ntm, ntn = (M + 255) // 256, (N + 255) // 256
    assert ntm * ntn > cus(), "the case no longer has more tiles than compute units"
    assert ((ntn % 4 == 0 and ntn >= 8 and ntm % 2 == 0) == (N == WRES[1])) and (N == WRES[1] or ((ntm * ntn) % 8 != 0 and ntm % 4 != 0))
    run_exact_public(ctx, dt, M, N, K, (BIAS, BIAS_RESID), f"walk {M}x{N}x{K} {DTN[dt]}")


DIRECT_WALK = (64 * 256 + 129, 1024)               # 65 x 4 tiles of the DIRECT instances (N = 1024 as in the tower)
CONSUMER = [(1, 264, 128), (128, 128, 256), (383, 376, 192), (511, 448, 128), (257, 64, 448), (*DIRECT_WALK, 128), (*DIRECT_WALK, 192), (*WRES, 256), (*WRES, 384)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K", CONSUMER, ids=[f"{m}x{n}x{k}" for m, n, k in CONSUMER])
def test_exact_ln_consumer(ctx, dt, M, N, K):
    """EPI_LN_BIAS with rstd a power of two, integer mean, colsum and bias: bitwise after one rounding.  nk = 2 (empty middle loop, the
    statistics prefetch right behind the first K-step) and nk = 3 inside multi-tile walks, W-resident order at nk = 4 and 6, ragged M and N,
    NaN guard rows behind rowstat."""
    a, w, _, _, acc = int_case(M, N, K)
    g = gen(M + N + K + 1)
    mean, s, b = ints((M, 1), 8, g), ints((1, N), 16, g), ints((1, N), 32, g)
    rstd = torch.exp2(-torch.randint(0, 7, (M, 1), generator=g, device=DEV).double())
    want = (rstd * (acc - mean * s) + b).to(dt)
    rowstat = torch.full((M + GUARD, 2), NAN, dtype=torch.float32, device=DEV)
    rowstat[:M, 0], rowstat[:M, 1] = mean[:, 0].float(), rstd[:, 0].float()
    A, W = padded(a.to(dt), 8), padded(w.to(dt), 16)
    if M > 5000:
        assert ((M + 255) // 256) * ((N + 255) // 256) > cus(), "the case no longer has more tiles than compute units"
    first = None
    for _ in range(2):
        o = Embedded(M, N, dt, gcols=4, offset=4)
        gemm_ex(ctx, dt, LN_BIAS, A, W, o.view, M, N, K, bias=b[0].float().contiguous(), rowstat=rowstat, colsum=s[0].float().contiguous())
        tag = f"consumer {M}x{N}x{K} {DTN[dt]}"
        assert o.guards_untouched(), f"{tag}: guards of the output buffer were written"
        assert torch.isfinite(o.view.float()).all(), f"{tag}: non-finite output"
        assert_bits(o.view, want, tag)
        if first is None:
            first = o.view.clone()
        else:
            assert_bits(o.view, first, f"{tag} against the first launch")


PRODUCER = [(1, 64, 128, "both"), (128, 320, 128, "mean"), (383, 320, 192, "both"), (511, 448, 128, "mean"), (385, 448, 448, "none"), (257, 1024, 256, "none"),
            (300, 64, 384, "mean"), (*DIRECT_WALK, 128, "both"), (*DIRECT_WALK, 192, "both")]


def run_producer(ctx, dt, M, N, K, A, W, bias, old, gnext, rowmean, cshift):
    """One producer launch on NaN-guarded buffers; returns (resid Embedded, x16 Embedded, stats [planes, M, 2], planes written)."""
    NP, planes = N // 64, ((N + 255) // 256) * 4 + 2
    res = Embedded(M, N, torch.float32, init=old, gcols=4)
    x16 = Embedded(M, N, dt, gcols=4, offset=4)
    stats = torch.full((planes, M, 2), NAN, dtype=torch.float32, device=DEV)
    gemm_ex(ctx, dt, LNOUT, A, W, res.view, M, N, K, bias=bias, gnext=gnext, x16=x16.view, stats=stats, rowmean=rowmean, cshift=cshift)
    return res, x16, stats, NP


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K,mode", PRODUCER, ids=[f"{m}x{n}x{k}-{c}" for m, n, k, c in PRODUCER])
def test_exact_ln_producer(ctx, dt, M, N, K, mode):
    """EPI_BIAS_RESID_LNOUT with gnext powers of two and integer rowmean / cshift: the new residual, x16 and EVERY partial (sum, sum of squares)
    bitwise; N in {64, 320, 448} (a wave with no valid column, or half) and 1024; centre 0 (rowmean NULL, cshift given and ignored), rowmean
    alone, rowmean + cshift; ldx16 > N; guard rows, columns and pieces untouched."""
    a, w, b, old, acc = int_case(M, N, K)
    g = gen(M + N + K + 2)
    gn = torch.exp2(torch.randint(-3, 2, (N,), generator=g, device=DEV).double())
    rm = ints((M + GUARD,), 16, g)
    rm[M:] = NAN
    csh = torch.tensor([3.0], device=DEV)
    c = {"none": torch.zeros(M, 1, dtype=torch.float64, device=DEV), "mean": rm[:M, None], "both": rm[:M, None] + 3.0}[mode]
    rnew = old + acc + b
    d = rnew - c
    NP = N // 64
    want_part = torch.stack([d.view(M, NP, 64).sum(-1), (d * d).view(M, NP, 64).sum(-1)], -1).transpose(0, 1).contiguous()
    assert float(want_part[..., 1].max()) < 2 ** 24 and float(d.abs().max()) < 4096, "a sum of squares may leave fp32's integer range"
    A, W = padded(a.to(dt), 8), padded(w.to(dt), 16)
    first = None
    for _ in range(2):
        res, x16, stats, _ = run_producer(ctx, dt, M, N, K, A, W, b.float(), old.float(), gn.float(), None if mode == "none" else rm.float(),
                                          None if mode == "mean" else csh)
        tag = f"producer {M}x{N}x{K} {mode} {DTN[dt]}"
        assert res.guards_untouched() and x16.guards_untouched(), f"{tag}: guards of the residual or of x16 were written"
        assert torch.isnan(stats[NP:]).all(), f"{tag}: partial statistics written behind piece {NP - 1}"
        assert_bits(res.view, rnew.float(), f"{tag} residual")
        assert_bits(x16.view, (d * gn).to(dt), f"{tag} x16")
        ne = bits(stats[:NP]) != bits(want_part.float())
        if ne.any():
            p, r, j = [int(v) for v in ne.nonzero()[0]]
            raise AssertionError(f"{tag}: {int(ne.sum())} partial statistics differ; first at piece {p} ({where(r, p * 64)}) {'sum' if j == 0 else 'sum of squares'}: "
                                 f"got {float(stats[p, r, j])!r} want {float(want_part[p, r, j])!r}")
        if first is None:
            first = (res.view.clone(), x16.view.clone(), stats.clone())
        else:
            assert torch.equal(bits(res.view), bits(first[0])) and torch.equal(bits(x16.view), bits(first[1])) and torch.equal(bits(stats), bits(first[2])), \
                f"{tag}: a second launch gives different bits"


# --------------------------------------------------------------------------------------------------
# 2. bound tests
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def real_case(M, N, K, dt):
    g = gen(M * 13 + N * 5 + K + MANT[dt])
    a = torch.randn(M, K, generator=g, device=DEV).to(dt)
    w = (torch.randn(N, K, generator=g, device=DEV) * (1.5 / math.sqrt(K))).to(dt)
    b = torch.randn(N, generator=g, device=DEV)
    old = 2.0 * torch.randn(M, N, generator=g, device=DEV)
    a64, w64 = a.double(), w.double()
    acc = a64 @ w64.t()
    Eacc = K * UACC * (a64.abs() @ w64.abs().t())
    return a, w, b, old, acc, Eacc


BOUND_SHAPES = [(257, 320, 128), (385, 448, 192), (*WRES, 256)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K", BOUND_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in BOUND_SHAPES])
def test_bound_public_epilogues(ctx, dt, M, N, K):
    """Random real inputs, all seven public epilogues, row-major and blocked W: every element within the derived bound (module docstring)."""
    a, w, b, old, acc, Eacc = real_case(M, N, K, dt)
    A, W, Wb = padded(a, 8), padded(w, 16), pack_blocked(ctx, w)
    b64 = b.double()
    pre, Epre = acc + b64, rnd(acc + b64, Eacc)
    for epi in (NONE, BIAS, QGELU, GELU, RESID, BIAS_RESID, SWIGLU, F32):
        out32 = epi in (RESID, BIAS_RESID, F32)
        x, Ex = (acc, Eacc) if epi in (NONE, RESID, SWIGLU) else (pre, Epre)
        if epi in (NONE, BIAS, F32):
            ref, E = x, Ex
        elif epi == QGELU:
            ref, E = quick_gelu_ref(x), quick_gelu_bound(x, Ex)
        elif epi == GELU:
            ref, E = gelu_ref(x), gelu_bound(x, Ex)
        elif epi in (RESID, BIAS_RESID):
            ref = old.double() + x
            E = rnd(ref, Ex)
        else:                                      # W rows interleaved [32 gate | 32 up] per 64
            xg, xu = x.view(M, N // 64, 2, 32)[:, :, 0].reshape(M, N // 2), x.view(M, N // 64, 2, 32)[:, :, 1].reshape(M, N // 2)
            eg, eu = Ex.view(M, N // 64, 2, 32)[:, :, 0].reshape(M, N // 2), Ex.view(M, N // 64, 2, 32)[:, :, 1].reshape(M, N // 2)
            ref, E = silu_ref(xg) * xu, swiglu_bound(xg, eg, xu, eu)
        if not out32:
            E = E + hulp(ref.abs() + E, dt)
        No = N // 2 if epi == SWIGLU else N
        prev = None
        for layout in ("row", "blk"):
            o = Embedded(M, No, torch.float32 if out32 else dt, init=old if epi in (RESID, BIAS_RESID) else None)
            gemm_ex(ctx, dt, epi, A, Wb if layout == "blk" else W, o.view, M, N, K, bias=None if epi in (NONE, RESID, SWIGLU) else b, blocked=layout == "blk")
            tag = f"bound {M}x{N}x{K} {EPN[epi]} {layout} {DTN[dt]}"
            assert o.guards_untouched(), f"{tag}: guards written"
            assert_bound(o.view, ref, E, tag, (EPN[epi], DTN[dt]))
            if prev is not None:
                assert_bits(o.view, prev, f"{tag} against row-major W")
            prev = o.view.clone()


LN_BOUND_SHAPES = [(385, 448, 192), (*DIRECT_WALK, 128)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,N,K", LN_BOUND_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in LN_BOUND_SHAPES])
def test_bound_ln_instances(ctx, dt, M, N, K):
    """The three folded-LayerNorm instances on random real inputs: consumer (plain, QuickGELU) against rstd (acc - mean s) + b in float64,
    producer's residual, x16 and every partial statistic, each element within its derived bound."""
    a, w, b, old, acc, Eacc = real_case(M, N, K, dt)
    A, W = padded(a, 8), padded(w, 16)
    g = gen(M + N + K + 3)
    mean = torch.randn(M, 1, generator=g, device=DEV) * 3.0
    rstd = 0.25 + 2.0 * torch.rand(M, 1, generator=g, device=DEV)
    s = torch.randn(1, N, generator=g, device=DEV)
    rowstat = torch.cat([mean, rstd], 1).contiguous()
    lin, Elin = consumer_bound(acc, Eacc, mean.double(), rstd.double(), s.double(), b.double()[None])
    for epi, ref, E in ((LN_BIAS, lin, Elin), (LN_QGELU, quick_gelu_ref(lin), quick_gelu_bound(lin, Elin))):
        E = E + hulp(ref.abs() + E, dt)
        o = Embedded(M, N, dt, offset=4)
        gemm_ex(ctx, dt, epi, A, W, o.view, M, N, K, bias=b, rowstat=rowstat, colsum=s[0].contiguous())
        assert o.guards_untouched()
        assert_bound(o.view, ref, E, f"bound {M}x{N}x{K} {EPN[epi]} {DTN[dt]}", (EPN[epi], DTN[dt]))
    N64 = N // 64 * 64                             # the producer needs whole pieces: the leading N64 columns of the same matrices
    gn = (1.0 + 0.3 * torch.randn(N64, generator=g, device=DEV))
    rm = 2.0 * torch.randn(M, generator=g, device=DEV)
    csh = torch.tensor([0.37], device=DEV)
    res, x16, stats, NP = run_producer(ctx, dt, M, N64, K, A, W[:N64], b[:N64].contiguous(), old[:, :N64], gn, rm, csh)
    assert res.guards_untouched() and x16.guards_untouched() and torch.isnan(stats[NP:]).all()
    c = (rm + csh).double()[:, None]               # the kernel's own single fp32 addition
    pre = acc[:, :N64] + b.double()[:N64]
    rnew = old.double()[:, :N64] + pre
    Er = rnd(rnew, rnd(pre, Eacc[:, :N64]))
    x, Ex16, t1, E1, t2, E2 = producer_bound(rnew, Er, c, gn.double(), dt, NP)
    tag = f"bound {M}x{N64}x{K} {EPN[LNOUT]} {DTN[dt]}"
    assert_bound(res.view, rnew, Er, tag + " residual", ("LNOUT resid", DTN[dt]))
    assert_bound(x16.view, x, Ex16, tag + " x16", ("LNOUT x16", DTN[dt]))
    assert_bound(stats[:NP, :, 0].t(), t1, E1, tag + " sums (col = piece)", ("LNOUT sum", DTN[dt]))
    assert_bound(stats[:NP, :, 1].t(), t2, E2, tag + " sums of squares (col = piece)", ("LNOUT sumsq", DTN[dt]))


def ln_stats(ctx, part, rowstat, rowmean, cshift, rows, NP, cols, eps, ok=True):
    from video_llava_amd import _lib
    rc = ctx.lib.pgv_ln_stats(ctx.handle, ptr(part), ptr(rowstat), ptr(rowmean), ptr(cshift), rows, NP, cols, eps, _lib.stream_ptr())
    torch.cuda.synchronize()
    if ok:
        _lib.check(rc, "pgv_ln_stats")
    return rc


@gpu
@pytest.mark.parametrize("NP", [1, 5, 16])
@pytest.mark.parametrize("with_shift", [False, True], ids=["noshift", "shift"])
def test_ln_stats_vs_fp64(ctx, NP, with_shift):
    """ln_stats_kernel on caller partials: (delta, rstd) and the updated rowmean against float64 within the derived bound, on rows with
    |delta| / sigma from 0 to 20, rows of variance 0 and an all-zero row; more than one block of rows; guard rows untouched."""
    M, cols = 515, NP * 64
    t1, t2, _ = _stats_case(M, NP, DEV, NP)
    part = torch.stack([t1, t2], -1).transpose(0, 1).contiguous()                # [NP][M][2]
    rowstat = torch.full((M + GUARD, 2), NAN, dtype=torch.float32, device=DEV)
    rm0 = torch.randn(M, generator=gen(NP), device=DEV) * 4.0
    rowmean = torch.full((M + GUARD,), NAN, dtype=torch.float32, device=DEV)
    rowmean[:M] = rm0
    csh = torch.tensor([-0.81], device=DEV) if with_shift else None
    ln_stats(ctx, part, rowstat, rowmean, csh, M, NP, cols, EPS)
    assert torch.isnan(rowstat[M:]).all() and torch.isnan(rowmean[M:]).all(), "guard rows written"
    z = torch.zeros(M, NP, dtype=torch.float64, device=DEV)
    delta, Edl, rstd, Er = ln_stats_bound(t1.double(), z, t2.double(), z, cols, EPS)
    tag = f"ln_stats np={NP} {'shift' if with_shift else 'noshift'}"
    assert_bound(rowstat[:M, :1], delta[:, None], Edl[:, None], tag + " delta", ("ln_stats delta", "f32"))
    assert_bound(rowstat[:M, 1:], rstd[:, None], Er[:, None], tag + " rstd", ("ln_stats rstd", "f32"))
    shift = -0.81 if with_shift else 0.0
    step = delta + float(np.float32(shift))
    want = rm0.double() + step
    assert_bound(rowmean[:M, None], want[:, None], rnd(want, rnd(step, Edl))[:, None], tag + " rowmean", ("ln_stats rowmean", "f32"))


# --------------------------------------------------------------------------------------------------
# 3. the folded LayerNorm as a chain
# --------------------------------------------------------------------------------------------------
CHAIN = [(300, 1024, 128, 320), (385, 320, 192, 264)]          # rows, LayerNorm width C, K of the producer GEMM, N of the consumer GEMM


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("M,C,K,N2", CHAIN, ids=[f"{m}x{c}" for m, c, k, n in CHAIN])
def test_folded_layernorm_chain_vs_fp64(ctx, dt, M, C, K, N2):
    """producer -> ln_stats -> consumer on caller buffers, twice in sequence (rowmean carried from the first sublayer to the second),
    against float64 LayerNorm(resid + A W^T + b) W2^T + b2: rows with |mean| / sigma up to 20, ragged M, C = 1024 and 320; colsum and b' are
    computed in float64 by the test.  Every output element, the row means and the statistics within the bound of the module docstring."""
    g = gen(M + C + K + MANT[dt])
    NP = C // 64
    sig = 0.5 + torch.rand(M, 1, generator=g, device=DEV, dtype=torch.float64)
    mu = sig * torch.linspace(-20, 20, M, device=DEV, dtype=torch.float64)[:, None]
    r_k = (mu + sig * torch.randn(M, C, generator=g, device=DEV, dtype=torch.float64)).float()      # the fp32 residual the kernels update
    r_ref, Er = r_k.double(), torch.zeros(M, C, dtype=torch.float64, device=DEV)
    rowmean = r_ref.mean(1).float()                 # any centre is valid: the previous row mean, as the tower keeps it
    res = Embedded(M, C, torch.float32, init=r_k, gcols=4)
    for layer in range(2):
        a = torch.randn(M, K, generator=g, device=DEV).to(dt)
        w = (torch.randn(C, K, generator=g, device=DEV) * (0.5 / math.sqrt(K))).to(dt)
        b = 0.3 * torch.randn(C, generator=g, device=DEV) + 0.5
        gamma = 1.0 + 0.2 * torch.randn(C, generator=g, device=DEV)
        beta = 0.1 * torch.randn(C, generator=g, device=DEV)
        w2 = (torch.randn(N2, C, generator=g, device=DEV) * (1.0 / math.sqrt(C))).to(dt)
        b2 = torch.randn(N2, generator=g, device=DEV)
        csh = b.double().mean().float().reshape(1)
        colsum64 = w2.double() @ gamma.double()
        bf64 = b2.double() + w2.double() @ beta.double()
        colsum, bf = colsum64.float(), bf64.float()
        # ---- kernels
        x16 = Embedded(M, C, dt, gcols=8)            # ldx16 = lda of the consumer = C + 8
        stats = torch.full((NP + 2, M, 2), NAN, dtype=torch.float32, device=DEV)
        rowstat = torch.full((M + GUARD, 2), NAN, dtype=torch.float32, device=DEV)
        c = (rowmean + csh).double()[:, None]       # the producer's centre: one fp32 addition, reproduced here
        gemm_ex(ctx, dt, LNOUT, padded(a, 8), padded(w, 8), res.view, M, C, K, bias=b, gnext=gamma, x16=x16.view, stats=stats, rowmean=rowmean, cshift=csh)
        ln_stats(ctx, stats, rowstat, rowmean, csh, M, NP, C, EPS)
        out = Embedded(M, N2, dt, gcols=4, offset=4)
        gemm_ex(ctx, dt, LN_BIAS, x16.view, padded(w2, 8), out.view, M, N2, C, bias=bf, rowstat=rowstat, colsum=colsum)
        assert res.guards_untouched() and x16.guards_untouched() and out.guards_untouched() and torch.isnan(stats[NP:]).all() and torch.isnan(rowstat[M:]).all()
        # ---- float64 reference and bound
        acc = a.double() @ w.double().t()
        Eacc = K * UACC * (a.double().abs() @ w.double().abs().t())
        pre = acc + b.double()
        r_ref = r_ref + pre
        Er = rnd(r_ref, rnd(pre, Eacc) + Er)
        x, Ex16, t1, E1, t2, E2 = producer_bound(r_ref, Er, c, gamma.double(), dt, NP)
        delta, Edl, rstd_c, Erstd = ln_stats_bound(t1, E1, t2, E2, C, EPS)
        want = layer_norm_linear(r_ref, gamma.double(), beta.double(), w2.double(), b2.double(), EPS)
        model = folded_ln_model(r_ref, gamma.double(), beta.double(), w2.double(), b2.double(), c, EPS)
        assert float((model - want).abs().max() / want.abs().max()) < 1e-10, "the float64 split disagrees with layer_norm + Linear"
        rstd = rstd_c[:, None]
        Z = (want - bf64) / rstd
        w2a = w2.double().abs()
        E_in = Erstd[:, None] * Z.abs() + (rstd + Erstd[:, None]) * (Ex16 @ w2a.t() + Edl[:, None] * colsum64.abs())
        E_in = E_in + rstd * delta.abs()[:, None] * U32 * colsum64.abs() + U32 * bf64.abs()
        acc2 = x @ w2.double().t()
        Eacc2 = C * UACC * ((x.abs() + Ex16) @ w2a.t())
        _, E_own = consumer_bound(acc2, Eacc2, delta[:, None], rstd, colsum64[None], bf64[None])
        E = E_in + E_own
        E = E + hulp(want.abs() + E, dt)
        tag = f"chain {M}x{C} layer {layer} {DTN[dt]}"
        assert_bound(res.view, r_ref, Er, tag + " residual", ("chain resid", DTN[dt]))
        assert_bound(rowstat[:M, :1], delta[:, None], Edl[:, None], tag + " delta", ("chain delta", DTN[dt]))
        assert_bound(rowstat[:M, 1:], rstd, Erstd[:, None], tag + " rstd", ("chain rstd", DTN[dt]))
        mean_ref = r_ref.mean(1)
        step = delta + csh.double()
        assert_bound(rowmean[:, None], mean_ref[:, None], (rnd(mean_ref, rnd(step, Edl)) + U32 * c[:, 0].abs())[:, None], tag + " rowmean", ("chain rowmean", DTN[dt]))
        assert_bound(out.view, want, E, tag + " output", ("chain out", DTN[dt]))
        # a broken split must leave this bound (the centre is far from zero on most rows)
        for defect in ("no_centre", "mean_for_delta"):
            bad = folded_ln_model(r_ref, gamma.double(), beta.double(), w2.double(), b2.double(), c, EPS, defect)
            assert (~((bad - want).abs() <= E)).any(1).double().mean() > 0.8, defect


# --------------------------------------------------------------------------------------------------
# 4. refusals
# --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
def test_gemm_refuses_what_it_cannot_run(ctx, dt):
    """Every unsupported call returns PGV_EINVAL and leaves the outputs as they were."""
    from video_llava_amd import _lib
    M, N, K = 40, 128, 128
    a = torch.zeros(M + 1, K + 8, dtype=dt, device=DEV)
    w = torch.zeros(N + 1, K + 8, dtype=dt, device=DEV)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    bias, rowstat, colsum, gnext = f(N), f(2 * M), f(N), f(N)
    c16 = torch.full((M * (N + 8) + 8,), NAN, dtype=dt, device=DEV)
    c32 = torch.full((M * (N + 8) + 8,), NAN, dtype=torch.float32, device=DEV)
    x16 = torch.full((M * (N + 8),), NAN, dtype=dt, device=DEV)
    stats = torch.full((2 * N // 64 * M * 2,), NAN, dtype=torch.float32, device=DEV)
    A, W = a[:M, :K], w[:N, :K]
    ln = dict(bias=bias, rowstat=rowstat, colsum=colsum)
    po = dict(bias=bias, gnext=gnext, x16=x16, stats=stats, ldx16=N)
    cases = [
        ("K % 64", dict(epi=BIAS, K=96)),
        ("N % 8", dict(epi=BIAS, N=124)),
        ("lda % 8", dict(epi=BIAS, lda=K + 4)),
        ("ldw % 8", dict(epi=BIAS, ldw=K + 4)),
        ("A misaligned", dict(epi=BIAS, A=a[:M, 4:K + 4])),
        ("W misaligned", dict(epi=BIAS, W=w[:N, 4:K + 4])),
        ("C16 misaligned", dict(epi=BIAS, C=c16[2:])),
        ("C32 misaligned", dict(epi=F32, C=c32[2:])),
        ("ldc % 4", dict(epi=BIAS, ldc=N + 2)),
        ("consumer K = 64", dict(epi=LN_BIAS, K=64, **ln)),
        ("consumer QuickGELU K = 64", dict(epi=LN_QGELU, K=64, **ln)),
        ("producer K = 64", dict(epi=LNOUT, K=64, **po)),
        ("consumer blocked W", dict(epi=LN_BIAS, blocked=True, **ln)),
        ("producer blocked W", dict(epi=LNOUT, blocked=True, **po)),
        ("consumer without rowstat", dict(epi=LN_BIAS, bias=bias, colsum=colsum)),
        ("producer N % 64", dict(epi=LNOUT, N=96, **po)),
        ("producer ldx16 % 4", dict(epi=LNOUT, **{**po, "ldx16": N + 2})),
        ("blocked N % 16", dict(epi=BIAS, N=120, blocked=True)),
        ("unknown epilogue", dict(epi=11)),
        ("negative epilogue", dict(epi=-1)),
        ("empty", dict(epi=BIAS, M=0)),
    ]
    for name, kw in cases:
        kw = dict(kw)
        epi = kw.pop("epi")
        out32 = epi in (RESID, BIAS_RESID, F32, LNOUT)
        args = dict(A=A, W=W, C=(c32 if out32 else c16), M=M, N=N, K=K, ldc=N + 8)
        args.update(kw)
        rc = gemm_ex(ctx, dt, epi, args.pop("A"), args.pop("W"), args.pop("C"), args.pop("M"), args.pop("N"), args.pop("K"), ok=False, **args)
        assert rc == _lib.PGV_EINVAL, f"{name}: accepted (rc {rc})"
        for t in (c16, c32, x16, stats):
            assert torch.isnan(t.float()).all(), f"{name}: a refused call wrote to an output"
    # a null bias stands on a vector of 65536 zeros: wider outputs must bring their own
    Nw = 65536 + 8
    ww = torch.zeros(Nw, 64, dtype=dt, device=DEV)
    cw = torch.full((Nw,), NAN, dtype=dt, device=DEV)
    assert gemm_ex(ctx, dt, NONE, a[:1, :64], ww, cw, 1, Nw, 64, ldc=Nw, ok=False) == _lib.PGV_EINVAL and torch.isnan(cw.float()).all()
    assert ln_stats(ctx, stats, None, f(M), None, M, 2, 128, EPS, ok=False) == _lib.PGV_EINVAL
    assert ln_stats(ctx, stats, f(2 * M), f(M), None, M, 0, 128, EPS, ok=False) == _lib.PGV_EINVAL
