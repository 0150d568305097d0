"""The decode GEMV family (csrc/gemv.hip) element by element, as a decode step runs it: the residual + RMSNorm producer (16-row and 8-phase
forms), the consumers that scale their accumulators by rstd (store16, SwiGLU, f32), the greedy candidates of the head, the fragment-blocked
activation layout between them, and the two kernels that start a chain -- through the test entries pgv_gemv_ex / pgv_gemv_prep, which fill the
internal launcher exactly as decode does and report the launch shape that ran.  Tests marked `gpu` launch kernels; the others check the layout
codecs, the float64 models and the bounds themselves and run anywhere.

1. EXACT tests (integer inputs).  x and the old residual are integers (|x| <= 4, |r_old| <= 64), W integers in [-3, 3] (times a power-of-two row
scale for fp8 weights: on the e4m3 grid; without zeros but for a few planted ones for the 12-bit copy, whose exception list holds them), gamma
powers of two.  sum_k |x||w| and every sum of squares stay below 2^24 in units of their granularity (asserted on the host, `check_exact`), so
every fp32 sum is exact IN ANY ORDER: the new residual, xg = round16(r gamma) at its row-major or blocked address and every ssq_out[ct][rb][b]
(0 for b >= B) are compared bitwise with float64; so are store16 / f32 outputs without ssq_in.  With ssq_in (integer partials whose sum is
exact) the only inexact operations are ss * inv_h + eps (inv_h = fl32(1 / hidden): two roundings, then one more for + eps; an FMA only removes
one), rsqrtf (2 ulp, as in the ln_stats bound of test_gpu_gemm.py) and the multiply by rstd; SwiGLU adds sigmoid_mul_bound with the SiLU constant;
16-bit outputs add half an ulp.  The bound of every element is assembled from those alone.  Columns b >= B of x and ssq_in are NaN; every output
sits in a sentinel-filled allocation that is compared bitwise as a whole (guard zones, pad columns, xg slots of absent sequences); every launch
runs twice and must give the same bits; blocked and row-major x must give the same bits at 9 <= B <= 64.
The head candidates are checked against the logits the kernel stored: amax_val bitwise their maximum over the rows < N of the block, amax_idx
the smallest index attaining it (ties are everywhere with integer inputs; asserted), NaN never wins, an all-NaN block gives (-inf, 0x7fffffff).

2. CHAIN test (real inputs): prep or embed -> qkv consumer -> o_proj producer -> gate/up consumer -> down_proj producer -> head, each stage
reading the device buffers the previous one wrote, against float64 RMSNorm -> Linear from the same 16-bit weights.  Every element of every
intermediate is held to a bound propagated stage by stage (u = 2^-24):
  operand        x16 = round16(fl32(r gamma)): E_x = rnd(r gamma, |gamma| E_r) + half an ulp of the 16-bit type.
  accumulation   |acc - x_ref W^T| <= E_x |W|^T + K 2^-23 (|x_ref| + E_x) |W|^T (products exact, one rounding per addition in any order; 2^-23 as in
                 test_gpu_gemm.py).  fp32 residual: rnd(r_old + acc).
  partials       a producer's sum of 16 squares: one rounding per square, a tree of depth 4: sum (2 |r| E_r + E_r^2) + 6 u sum (|r| + E_r)^2;
                 the prep / embed kernels sum H squares in an unspecified order: H u sum r^2.
  rstd           the consumer adds the P partials in a fixed but unspecified order ((P - 1) u sum), t = fl(ss inv_h) with inv_h = fl32(1 / H),
                 v = fl(t + eps), rstd = v^-1/2 with v's interval propagated exactly and 2 ulp for rsqrtf.
  consumer       y = fl(acc rstd): rnd(y, |acc| E_rstd + rstd E_acc + E_acc E_rstd); SwiGLU: swiglu_bound on (gate, up); 16-bit: + half an ulp.
Nothing in a bound comes from the kernel's output.  The worst err / bound per stage and dtype is printed and tabulated in DESIGN.md.

Every case asserts the launch shape it was written for (on 256 compute units; on another device the case is skipped with the shape named).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from bounds import EPS, U32, UACC, ULP1, hulp, rnd, silu_ref, swiglu_bound

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = math.nan
DTYPES = [torch.float16, torch.bfloat16]
DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}
STORE16, RESID, SWIGLU, F32, RESIDNORM = 0, 1, 2, 3, 5
W16, FP8, W12 = 0, 1, 2
FMTN = ["w16", "fp8", "w12"]
BS = [1, 8, 9, 16, 17, 32, 33, 48, 64]
KS = [32, 64, 96, 192, 512 + 32, 1056]
NPARTS = [1, 2, 127, 128, 129, 320, 384]
NO_IDX = 0x7fffffff
G = 128                                           # guard elements on either side of every device buffer (>= 7 * 16: the seven row blocks past the matrix of the last eight-block head workgroup)

WORST = {}                                        # (stage, dtype) -> worst err / bound seen


def col_tiles(B):
    return 1 if B <= 16 else (2 if B <= 32 else 4)


def xblk_tiles(B):
    return 0 if B <= 8 else col_tiles(B)


def ceil16(n):
    return (n + 15) // 16 * 16


# --------------------------------------------------------------------------------------------------
# layout codecs, written from the documented layouts (include/pgv.h)
# --------------------------------------------------------------------------------------------------
def xblk_encode(x, ct, fill):
    """x [B, K] -> flat [K / 32][ct][4 k-groups][16 sequences][8 elements]; the slots of sequences >= B hold `fill`."""
    B, K = x.shape
    full = torch.full((ct * 16, K), fill, dtype=x.dtype, device=x.device)
    full[:B] = x
    return full.view(ct, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1)


def xblk_decode(flat, K, ct):
    """flat blocked buffer -> [ct * 16, K]."""
    return flat.view(K // 32, ct, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(ct * 16, K)


def tiles_encode(a, ct, ts, pad, fill):
    """a [parts, B] -> flat tile-major [ct][parts][16] with tile stride ts; sequences >= B hold `pad`, the rest of every tile `fill`."""
    parts, B = a.shape
    wide = torch.full((parts, ct * 16), pad, dtype=a.dtype, device=a.device)
    wide[:, :B] = a
    full = torch.full((ct, ts), fill, dtype=a.dtype, device=a.device)
    full[:, :parts * 16] = wide.view(parts, ct, 16).permute(1, 0, 2).reshape(ct, parts * 16)
    return full.reshape(-1)


def tiles_decode(flat, parts, ct, ts):
    """flat tile-major array -> [parts, ct * 16]."""
    return flat[:ct * ts].view(ct, ts)[:, :parts * 16].reshape(ct, parts, 16).permute(1, 0, 2).reshape(parts, ct * 16)


def swiglu_pack(gate, up):
    """gate, up [I, K] -> [2 I, K]: blocks of 64 rows = 32 gate rows | the matching 32 up rows."""
    I, K = gate.shape
    return torch.stack([gate.view(I // 32, 32, K), up.view(I // 32, 32, K)], 1).reshape(2 * I, K)


def swiglu_unpack(w):
    K = w.shape[1]
    v = w.view(-1, 2, 32, K)
    return v[:, 0].reshape(-1, K), v[:, 1].reshape(-1, K)


def test_blocked_activation_codec_follows_the_documented_layout():
    """Host only.  Element (b, k) sits at ((((k / 32) ct + b / 16) 4 + (k % 32) / 8) 16 + b % 16) 8 + k % 8; round trip; absent sequences keep the fill."""
    for B, K, ct in ((3, 32, 1), (16, 96, 1), (17, 64, 2), (33, 160, 4), (64, 64, 4)):
        x = torch.arange(B * K, dtype=torch.float64).view(B, K) + 1
        flat = xblk_encode(x, ct, -1.0)
        assert flat.numel() == ct * 16 * K
        for b in range(B):
            for k in range(K):
                off = ((((k // 32) * ct + b // 16) * 4 + (k % 32) // 8) * 16 + b % 16) * 8 + k % 8
                assert flat[off] == x[b, k]
        back = xblk_decode(flat, K, ct)
        assert torch.equal(back[:B], x) and (back[B:] == -1).all()


def test_tile_major_codec_follows_the_documented_layout():
    """Host only.  ssq [ct][parts][16] / amax [ct][ceil(N / 16)][16] with a tile stride: entry (part, b) at (b / 16) ts + part 16 + b % 16."""
    for parts, B, ts in ((1, 3, 16), (5, 16, 96), (7, 17, 7 * 16 + 16), (33, 40, 33 * 16), (2, 64, 48)):
        ct = col_tiles(B)
        a = torch.arange(parts * B, dtype=torch.float64).view(parts, B) + 1
        flat = tiles_encode(a, ct, ts, 0.0, -1.0)
        assert flat.numel() == ct * ts
        for p in range(parts):
            for b in range(B):
                assert flat[(b // 16) * ts + p * 16 + b % 16] == a[p, b]
        back = tiles_decode(flat, parts, ct, ts)
        assert torch.equal(back[:, :B], a) and (back[:, B:] == 0).all()
        assert int((flat == -1).sum()) == ct * (ts - parts * 16)


def test_swiglu_row_packing_round_trip():
    """Host only.  Packed row (n / 32) 64 + n % 32 is gate row n, 32 rows further up row n."""
    I, K = 96, 8
    gate, up = torch.arange(I * K, dtype=torch.float64).view(I, K), -torch.arange(I * K, dtype=torch.float64).view(I, K) - 1
    w = swiglu_pack(gate, up)
    for n in range(I):
        assert torch.equal(w[(n // 32) * 64 + n % 32], gate[n]) and torch.equal(w[(n // 32) * 64 + n % 32 + 32], up[n])
    g2, u2 = swiglu_unpack(w)
    assert torch.equal(g2, gate) and torch.equal(u2, up)


# --------------------------------------------------------------------------------------------------
# float64 models and bounds
# --------------------------------------------------------------------------------------------------
def rstd_bound(ss, Ess, hidden, eps):
    """rsqrtf(ss * fl32(1 / hidden) + eps) from a sum of squares known to Ess: (rstd, bound)."""
    t = ss / hidden
    Et = Ess / hidden + 2 * U32 * (t + Ess / hidden)
    v = t + eps
    Ev = rnd(v, Et)
    rstd = v ** -0.5
    Er = (v - Ev).clamp_min(1e-300) ** -0.5 - rstd
    return rstd, Er + 2 * ULP1 * (rstd + Er)


def scaled_bound(acc, Eacc, rstd, Er):
    """y = fl32(acc * rstd[b]) for acc [B, N] known to Eacc and rstd [B] known to Er."""
    y = acc * rstd[:, None]
    return y, rnd(y, acc.abs() * Er[:, None] + rstd[:, None] * Eacc + Eacc * Er[:, None])


def swiglu_cols(y, E):
    """[B, 2 I] in the packed row order -> SwiGLU output [B, I] and its bound."""
    B = y.shape[0]
    yv, Ev = y.view(B, -1, 2, 32), E.view(B, -1, 2, 32)
    g, u, Eg, Eu = yv[:, :, 0].reshape(B, -1), yv[:, :, 1].reshape(B, -1), Ev[:, :, 0].reshape(B, -1), Ev[:, :, 1].reshape(B, -1)
    return silu_ref(g) * u, swiglu_bound(g, Eg, u, Eu)


def rms_norm_linear(r, gamma, W, eps):
    """HF's LlamaRMSNorm followed by the Linear, in float64."""
    return (r * (r.pow(2).mean(-1, keepdim=True) + eps) ** -0.5 * gamma) @ W.t()


def test_folded_rms_norm_model_and_its_bound():
    """Host only.  W (r rstd gamma) = rstd (W (r gamma)) to 1e-13 in float64; the rstd bound covers an fp32 evaluation and rejects a dropped,
    a double-counted partial and a neighbouring column's statistics."""
    g = torch.Generator().manual_seed(3)
    B, H, N = 5, 256, 48
    r, gamma, W = torch.randn(B, H, generator=g, dtype=torch.float64) * 3, 1 + 0.2 * torch.randn(H, generator=g, dtype=torch.float64), torch.randn(N, H, generator=g, dtype=torch.float64)
    want = rms_norm_linear(r, gamma, W, 1e-5)
    parts = (r * r).view(B, H // 16, 16).sum(-1)
    rstd = (parts.sum(-1) / H + 1e-5) ** -0.5
    got = ((r * gamma) @ W.t()) * rstd[:, None]
    assert float((got - want).abs().max() / want.abs().max()) < 1e-13
    for nparts in NPARTS:
        p = ssq_partials(nparts, 64, 5)
        ss = p.sum(0)
        hidden = 16 * nparts
        ref, Er = rstd_bound(ss, torch.zeros_like(ss), hidden, EPS)
        f32 = torch.rsqrt(ss.float() * torch.tensor(1.0 / hidden, dtype=torch.float32) + torch.tensor(EPS, dtype=torch.float32)).double()
        assert ((f32 - ref).abs() <= Er).all()
        bad = [((ss - p[-1]) / hidden + EPS) ** -0.5, ((ss + p[0]) / hidden + EPS) ** -0.5, ref.roll(1)]
        for b in bad:
            assert ((b - ref).abs() > 100 * Er).all(), nparts


def ssq_partials(nparts, ncols, seed):
    """Integer sum-of-squares partials [nparts, ncols] (float64): per column a different magnitude, exact column sums (< 2^24)."""
    g = torch.Generator().manual_seed(seed * 1000 + nparts)
    top = (2 ** 24 - 1) // nparts - 1
    scale = (torch.arange(ncols, dtype=torch.float64) % 16 + 1) / 16 * (1 - (torch.arange(ncols) // 16).double() / 8)
    p = 1 + torch.floor((0.5 + 0.5 * torch.rand(nparts, ncols, generator=g, dtype=torch.float64)) * top * scale)      # no partial is negligible
    assert float(p.sum(0).max()) < 2 ** 24
    return p


def check_exact(x, wi, q=1.0, r=None):
    """The exactness conditions: sum |x||w| (W in units of its row scale) below 2^24; with a residual r of granularity q, r and every sum of
    squares over 16 rows below 2^24 in units of q and q^2."""
    assert float((x.abs() @ wi.abs().t()).max()) < 2 ** 24, "a partial sum may leave fp32's integer range"
    if r is not None:
        assert float(r.abs().max()) / q < 2 ** 12, "a square may not be exact in fp32"
        assert float((r * r).view(r.shape[0], -1, 16).sum(-1).max()) / (q * q) < 2 ** 24, "a sum of squares may leave fp32's integer range"


@functools.lru_cache(maxsize=3)
def int_weights(N, K, fmt, swiglu=False, ties=False):
    """Integer weights [N, K] in [-3, 3] (float64, CPU) and the power-of-two row scale: 1 but for fp8 and for the up rows of a SwiGLU matrix (2^-6: silu(g) u
    of two accumulators of several hundred would leave fp16's range).  Large K: [-1, 1], so that the sums of
    squares stay exact.  ties: repeated rows inside a row block, so that the candidates' tie-break decides.  12-bit: no zeros (a zero's exponent lies outside every row window) except two planted per row for the exception list."""
    g = torch.Generator().manual_seed(N * 13 + K * 7 + fmt)
    lim = 3 if K <= 1056 else 1
    w = torch.randint(-lim, lim + 1, (N, K), generator=g).double()
    if fmt == W12:
        w = torch.where(w == 0, torch.full_like(w, float(lim)), w)
        w[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 0
        w[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 0
    rs = torch.exp2(torch.randint(-1, 1, (N,), generator=g).double()) if fmt == FP8 else torch.ones(N, dtype=torch.float64)
    if ties:                                       # the head: every third row block is one row sixteen times, every third has one row three times
        for j in range((N + 15) // 16):
            rows = torch.arange(16 * j, min(16 * j + 16, N))
            if j % 3 == 1:
                w[rows] = w[min(16 * j + 5, N - 1)].clone()
            elif j % 3 == 2:
                w[rows[rows % 16 == 9]], w[rows[rows % 16 == 14]] = w[16 * j + 2].clone(), w[16 * j + 2].clone()
    if swiglu:
        rs = torch.where(torch.arange(N) % 64 >= 32, rs / 64, rs)
    return w, rs


@functools.lru_cache(maxsize=6)
def int_x(K, positive=False):
    """Integer activations [64, K] in [-4, 4] ([-2, 2] at large K), rows distinct."""
    g = torch.Generator().manual_seed(K + 5)
    lim = 4 if K <= 1056 else 2
    x = torch.randint(-lim, lim + 1, (64, K), generator=g).double()
    if positive:
        x = x.abs().clamp_min(1)
    assert torch.unique(x, dim=0).shape[0] == 64, "repeated activation rows: a swapped column would go unnoticed"
    return x


def test_integer_cases_are_exact_in_fp32():
    """Host only.  Every (N, K, format) the exact tests use satisfies the exactness conditions at all 64 sequences, old residual included."""
    for fmt, N, K in sorted({(f, n, k) for f, n, k, *_ in PRODUCER16 + PRODUCER8}):
        wi, rs = int_weights(N, K, fmt)
        x = int_x(K)
        r = r_old_case(N) + (x @ wi.t()) * rs
        check_exact(x, wi, float(rs.min()), r)
    for mode, N, *_ in CONSUMER:
        for K in KS:
            check_exact(int_x(K), int_weights(N, K, W16)[0])


@functools.lru_cache(maxsize=4)
def r_old_case(N):
    g = torch.Generator().manual_seed(N + 11)
    return torch.randint(-64, 65, (64, N), generator=g).double()


# --------------------------------------------------------------------------------------------------
# device buffers and launch helpers
# --------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def ptr(t):
    return t.data_ptr() if t is not None else None


class Guarded:
    """n elements between two guard zones of G elements, all filled with `fill`; `want` starts as a copy and receives what the kernel is expected to
    write, so that one bitwise comparison covers guard zones, pad columns and the slots of absent sequences."""

    def __init__(self, n, dt, fill, init=None):
        self.buf = torch.full((n + 2 * G,), fill, dtype=dt, device=DEV)
        self.body = self.buf[G:G + n]
        if init is not None:
            self.body.copy_(init.reshape(-1).to(dt))
        self.before = self.buf.clone()

    def expect(self, want_body, what, mask=None, locate=None):
        want = self.before.clone()
        want[G:G + self.body.numel()] = want_body.reshape(-1).to(want.dtype)
        ne = bits(self.buf) != bits(want)
        if mask is not None:                       # mask: body elements whose content is unspecified
            ne[G:G + self.body.numel()] &= ~mask.reshape(-1)
        if ne.any():
            i = int(ne.nonzero()[0]) - G
            at = "a guard zone" if i < 0 or i >= self.body.numel() else (locate(i) if locate else f"element {i}")
            raise AssertionError(f"{what}: {int(ne.sum())} elements differ; first at offset {i} ({at}): got {float(self.buf[i + G])!r} want {float(want[i + G])!r}")

    def guards_ok(self):
        n = self.body.numel()
        return torch.equal(bits(self.buf[:G]), bits(self.before[:G])) and torch.equal(bits(self.buf[G + n:]), bits(self.before[G + n:]))


def rows2d(data, ld, dt, fill=NAN, extra_rows=0):
    """data [B, n] inside a `fill` buffer of row stride ld with `extra_rows` rows of fill below: (Guarded, view [B, n])."""
    B, n = data.shape
    g = Guarded((B + extra_rows) * ld, dt, fill)
    v = g.body.view(B + extra_rows, ld)
    v[:B, :n] = data.to(dt)
    g.before = g.buf.clone()
    return g, v


def overlay(g, B, ld, n, want):
    """The expected body of a rows2d buffer after the kernel wrote `want` [B, n]."""
    body = g.before[G:G + g.body.numel()].clone()
    body.view(-1, ld)[:B, :n] = want.to(body.dtype)
    return body


def loc2d(ld, what="row"):
    return lambda i: f"{what} {i // ld} col {i % ld} (row block {(i % ld) // 16})"


class Weights:
    """Device copies of an [N, K] matrix (float64 CPU, exactly representable): blocked 16-bit, or fp8 codes + row scales, or + the 12-bit copy."""

    def __init__(self, ctx, w, dt, fmt):
        from video_llava_amd import _lib
        N, K = w.shape
        Np, dc = ceil16(N), _lib.dtype_code(dt)
        wp = torch.zeros(Np, K, dtype=dt, device=DEV)
        wp[:N] = w.to(dt)
        assert torch.equal(torch.nan_to_num(wp[:N].double().cpu(), nan=12345.0), torch.nan_to_num(w, nan=12345.0)), "weights not representable in the 16-bit type"
        wb = torch.zeros(Np * K, dtype=dt, device=DEV)
        _lib.check(ctx.lib.pgv_pack_blocked(ctx.handle, dc, wp.data_ptr(), Np, K, wb.data_ptr(), _lib.stream_ptr()), "pgv_pack_blocked")
        self.W, self.scale, self.W12, self.fmt = wb, None, None, fmt
        if fmt == FP8:
            keep = wb.clone()
            w8, sc = torch.zeros(Np * K, dtype=torch.uint8, device=DEV), torch.zeros(Np, dtype=torch.float32, device=DEV)
            _lib.check(ctx.lib.pgv_quantize_fp8_blocked(ctx.handle, dc, wb.data_ptr(), w8.data_ptr(), sc.data_ptr(), Np, K, _lib.stream_ptr()), "quantize")
            assert torch.equal(bits(wb), bits(keep)), "the weights are not on the e4m3 grid of their row scale"
            self.W, self.scale = w8, sc
        elif fmt == W12:
            buf = torch.zeros(int(ctx.lib.pgv_w12_bytes(Np, K)), dtype=torch.uint8, device=DEV)
            counts = torch.zeros(Np // 16, dtype=torch.int32, device=DEV)
            _lib.check(ctx.lib.pgv_encode_w12_blocked(ctx.handle, dc, wb.data_ptr(), buf.data_ptr(), counts.data_ptr(), Np, K, _lib.stream_ptr()), "encode_w12")
            assert 0 < int(counts.max()) <= 64, "the 12-bit copy must hold exceptions, at most 64 per row block"
            self.W12 = buf
        torch.cuda.synchronize()


def gemv_ex(ctx, dt, mode, wt, x, ldx, out, ldo, N, K, B, ssq_in=None, nparts=0, hidden=1, eps=0.0, gamma=None, xg=None, ssq_out=None, amax_val=None,
            amax_idx=None, ssq_ts=0, amax_ts=0, k8=None, k8_bytes=None, x_blocked=True, ok=True):
    """One pgv_gemv_ex launch; returns (rc, (tl, ct, x2, k8, nwb, wfmt))."""
    from video_llava_amd import _lib
    d, sh = _lib.GemvDesc(), _lib.GemvShape(-1, -1, -1, -1, -1, -1)
    d.mode, d.d_W, d.d_wscale, d.d_W12 = mode, ptr(wt.W), ptr(wt.scale), ptr(wt.W12)
    d.d_x, d.ldx, d.d_out, d.ldo, d.N, d.K, d.B = ptr(x), ldx, ptr(out), ldo, N, K, B
    d.d_ssq_in, d.nparts_in, d.hidden, d.eps = ptr(ssq_in), nparts, hidden, eps
    d.d_gamma, d.d_xg, d.d_ssq_out, d.d_amax_val, d.d_amax_idx = ptr(gamma), ptr(xg), ptr(ssq_out), ptr(amax_val), ptr(amax_idx)
    d.ssq_ts, d.amax_ts, d.d_k8_part = ssq_ts, amax_ts, ptr(k8)
    d.k8_part_bytes = (k8.numel() * k8.element_size() if k8 is not None else 0) if k8_bytes is None else k8_bytes
    d.x_blocked, d.shape = 1 if x_blocked else 0, ctypes.pointer(sh)
    rc = ctx.lib.pgv_gemv_ex(ctx.handle, _lib.dtype_code(dt), ctypes.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    if ok:
        _lib.check(rc, "pgv_gemv_ex")
    return rc, (sh.tl, sh.ct, sh.x2, sh.k8, sh.nwb, sh.wfmt)


def gemv_prep(ctx, dt, tok, table, resid, gamma, xg, ssq, B, H, blocked, ok=True):
    """One pgv_gemv_prep launch: the embedding gather (tok, table given) or the prep of rows already in resid."""
    from video_llava_amd import _lib
    rc = ctx.lib.pgv_gemv_prep(ctx.handle, _lib.dtype_code(dt), ptr(tok), ptr(table), ptr(resid), ptr(gamma), ptr(xg), ptr(ssq), B, H, 1 if blocked else 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    if ok:
        _lib.check(rc, "pgv_gemv_prep")
    return rc


def assert_shape(ran, want, what):
    """The launch shape the case was written for.  On a device that is not 256 compute units wide the choice may differ: skip, naming the shape."""
    if ran != want:
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        msg = f"{what}: ran (tl, ct, x2, k8, nwb, wfmt) = {ran}, the case was written for {want}"
        if cu != 256:
            pytest.skip(f"{msg}; that shape cannot be selected on {cu} compute units")
        raise AssertionError(msg + " -- choose_gemv was retuned: move the case to a shape that selects this instance")


def assert_bound(got, ref, bound, what, key, locate):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.nan_to_num(torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))), nan=math.inf)
    worst, i = float(ratio.max()), int(ratio.argmax())
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound; worst at {locate(i)}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} "
                             f"bound {float(bound.flatten()[i]):.3e} (err / bound {worst:.3g})")


def report(prefix):
    print(f"\n[gemv] worst err/bound so far: {({f'{k[0]}/{k[1]}': round(v, 3) for k, v in WORST.items() if k[0].startswith(prefix)})}")


def same_bits(a, b):
    """Bitwise equality that lets any NaN match any NaN."""
    return bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def x_operand(x, B, K, dt, blocked):
    """The activation operand of a consumer on the device, columns b >= B NaN: blocked [K / 32][ct][4][16][8], or row-major with NaN pad columns and
    NaN rows below.  Returns (Guarded, pointer tensor, ldx)."""
    if blocked:
        g = Guarded(col_tiles(B) * 16 * K, dt, NAN, init=xblk_encode(x[:B].to(DEV), col_tiles(B), NAN))
        return g, g.body, K
    g, v = rows2d(x[:B].to(DEV), K + 8, dt, NAN, extra_rows=2)
    return g, v, K + 8


# --------------------------------------------------------------------------------------------------
# 1a. consumers: store16, SwiGLU, f32 (+ head candidates)
# --------------------------------------------------------------------------------------------------
# (mode, N, format, dtypes, Ks, Bs, {narrow B <= 16: tl, wide: tl})
NARROW, WIDE = [1, 8, 9, 16], [17, 32, 33, 48, 64]
CONSUMER = [
    (STORE16, 48, W16, DTYPES, KS, BS, {"n": 1, "w": 3}), (STORE16, 96, W12, [torch.bfloat16], [64, 192], NARROW, {"n": 1}),
    (STORE16, 64, W16, DTYPES, KS, BS, {"n": 1, "w": 4}), (STORE16, 80, W16, DTYPES, KS, WIDE, {"w": 1}),
    (STORE16, 64, FP8, DTYPES, [64, 192], BS, {"n": 1, "w": 4}),
    (STORE16, 6144, W16, DTYPES, [64], NARROW, {"n": 3}), (STORE16, 14336, W16, DTYPES, [64], NARROW, {"n": 4}),
    (SWIGLU, 64, W16, DTYPES, KS, BS, {"n": 2, "w": 4}), (SWIGLU, 192, W16, DTYPES, KS, NARROW, {"n": 2}), (SWIGLU, 128, W16, DTYPES, KS, WIDE, {"w": 4}),
    (SWIGLU, 192, FP8, DTYPES, [64, 192], BS, {"n": 2, "w": 4}), (SWIGLU, 64, W12, [torch.bfloat16], [64, 192], NARROW, {"n": 2}),
    (SWIGLU, 32 * 514, W16, DTYPES, [64, 192], WIDE, {"w": 6}), (SWIGLU, 32 * 514, FP8, DTYPES, [64, 192], WIDE, {"w": 6}),
    (SWIGLU, 32 * 770, W16, DTYPES, [64], WIDE, {"w": 8}), (SWIGLU, 32 * 770, FP8, DTYPES, [64], WIDE, {"w": 8}),
    (F32, 515, W16, DTYPES, KS, BS, {"n": 1, "n9": 8, "w": 8}), (F32, 520, W16, DTYPES, KS, [9, 16, 33, 64], {"n9": 8, "w": 8}),
    (F32, 515, FP8, DTYPES, [64, 192], BS, {"n": 1, "n9": 8, "w": 8}), (F32, 515, W12, [torch.bfloat16], [64], NARROW, {"n": 1, "n9": 8}),
]
CONSUMER_CASES = [(m, n, f, dt) for m, n, f, dts, *_ in CONSUMER for dt in dts]
MODEN = {STORE16: "store16", SWIGLU: "swiglu", F32: "f32", RESIDNORM: "producer"}


def want_tl(mode, tls, B):
    if B > 16:
        return tls["w"]
    return tls["n9"] if (B > 8 and "n9" in tls) else tls["n"]


def check_candidates(av, ai, logits, N, B, amax_ts, what, need_tie=False):
    """amax_val / amax_idx [ct][nrb][16] against the logits the kernel stored: per (row block, b < B) the largest non-NaN logit over rows < N and the
    smallest index attaining it; (-inf, 0x7fffffff) when there is none.  Entries of sequences >= B are unspecified; the gaps keep their bits."""
    nrb, ct = (N + 15) // 16, col_tiles(B)
    lg = torch.full((B, nrb * 16), -math.inf, dtype=torch.float32, device=DEV)
    lg[:, :N] = torch.nan_to_num(logits[:B, :N], nan=-math.inf)
    blk = lg.view(B, nrb, 16)
    val, arg = blk.max(-1)                                          # [B, nrb]
    first = (blk == val[..., None]).float().argmax(-1)            # smallest index of the maximum
    idx = torch.where(val > -math.inf, first + torch.arange(nrb, device=DEV)[None] * 16, torch.full_like(first, NO_IDX)).to(torch.int32)
    if need_tie:
        assert int(((blk == val[..., None]).sum(-1) > 1).sum()) > 0, f"{what}: no block has a tied maximum: the tie-break is not exercised"
    unspec = tiles_encode(torch.zeros(nrb, B, dtype=torch.bool, device=DEV), ct, amax_ts, True, False)
    av.expect(tiles_encode(val.t().contiguous(), ct, amax_ts, 0.0, NAN), what + " amax_val", unspec, lambda i: f"tile {i // amax_ts} row block {(i % amax_ts) // 16} b {i % 16}")
    ai.expect(tiles_encode(idx.t().contiguous(), ct, amax_ts, 0, -7), what + " amax_idx", unspec, lambda i: f"tile {i // amax_ts} row block {(i % amax_ts) // 16} b {i % 16}")


@gpu
@pytest.mark.parametrize("mode,N,fmt,dt", CONSUMER_CASES, ids=[f"{MODEN[m]}-{n}-{FMTN[f]}-{DTN[dt]}" for m, n, f, dt in CONSUMER_CASES])
def test_consumer_exact_accumulators_bounded_rstd(ctx, mode, N, fmt, dt):
    """Integer x and W: without ssq_in store16 and f32 are bitwise float64 (SwiGLU within the sigmoid's bound); with ssq_in every element is within
    the bound of ss * inv_h + eps, rsqrtf and the multiply.  nparts_in walks {1, 2, 127, 128, 129, 320, 384} over the (B, K) grid of the case;
    columns b >= B of x and ssq_in are NaN; blocked and row-major x give the same bits; every launch twice; f32 also checks the candidates."""
    _, _, _, _, Ks, Bs, tls = next(c for c in CONSUMER if c[:3] == (mode, N, fmt))
    No = N // 2 if mode == SWIGLU else N
    odt = torch.float32 if mode == F32 else dt
    ldo = No + (3 if mode == F32 else 4)
    nrb = (N + 15) // 16
    for iK, K in enumerate(Ks):
        wi, rs = int_weights(N, K, fmt, mode == SWIGLU, mode == F32)
        x64 = int_x(K)
        check_exact(x64, wi)
        wt = Weights(ctx, wi * rs[:, None], dt, fmt)
        acc_all = ((x64 @ wi.t()) * rs).to(DEV)
        for iB, B in enumerate(Bs):
            ct = col_tiles(B)
            tl = want_tl(mode, tls, B)
            k8_fmt = W12 if (fmt == W12 and ct == 1) else fmt
            shape = (tl, ct, int(B <= 8 and tl < 6), 0, 0, k8_fmt)
            nparts = NPARTS[(iB + iK) % len(NPARTS)]
            hidden = max(16 * nparts, 64)
            parts = ssq_partials(nparts, 64, K + N)
            ssq_ts = 16 * nparts + 16
            ssq_in = Guarded(ct * ssq_ts, torch.float32, NAN, init=tiles_encode(parts[:, :B].to(DEV), ct, ssq_ts, NAN, NAN))
            acc = acc_all[:B]
            rstd, Er = rstd_bound(parts[:, :B].sum(0).to(DEV), torch.zeros(B, dtype=torch.float64, device=DEV), hidden, EPS)
            amax_ts = 16 * nrb + 16
            tag = f"{MODEN[mode]} N={N} K={K} B={B} {FMTN[fmt]} {DTN[dt]}"
            for scaled in (False, True):
                if scaled:
                    y, Ey = scaled_bound(acc, torch.zeros_like(acc), rstd, Er)
                else:
                    y, Ey = acc, torch.zeros_like(acc)
                if mode == SWIGLU:
                    y, Ey = swiglu_cols(y, Ey)
                if odt != torch.float32:
                    Ey = Ey + hulp(y.abs() + Ey, dt)
                exact = not scaled and mode != SWIGLU
                first = None
                for blocked in ([True, False] if xblk_tiles(B) else [False]):
                    for rep in range(2):
                        xg_, xp, ldx = x_operand(x64, B, K, dt, blocked)
                        out = Guarded(B * ldo, odt, NAN)
                        av = Guarded(ct * amax_ts, torch.float32, NAN) if mode == F32 else None
                        ai = Guarded(ct * amax_ts, torch.int32, -7) if mode == F32 else None
                        _, ran = gemv_ex(ctx, dt, mode, wt, xp, ldx, out.body, ldo, N, K, B, ssq_in=ssq_in.body if scaled else None, nparts=nparts, hidden=hidden, eps=EPS,
                                         amax_val=av.body if av else None, amax_idx=ai.body if ai else None, ssq_ts=ssq_ts, amax_ts=amax_ts, x_blocked=blocked)
                        assert_shape(ran, shape, tag)
                        t2 = f"{tag} {'scaled' if scaled else 'plain'} {'blocked' if blocked else 'row-major'} x"
                        got = out.body.view(B, ldo)[:, :No]
                        if exact:
                            out.expect(overlay(out, B, ldo, No, y), t2, locate=loc2d(ldo, "b"))
                        else:
                            assert torch.isfinite(got.float()).all(), f"{t2}: non-finite output (a NaN column read, or an element not written)"
                            out.expect(overlay(out, B, ldo, No, got), t2 + " guards")
                            assert_bound(got, y, Ey, t2, (f"exact {MODEN[mode]}", DTN[dt]), loc2d(No, "b"))
                        if mode == F32:
                            check_candidates(av, ai, got, N, B, amax_ts, t2, need_tie=True)
                        assert xg_.guards_ok() and torch.equal(bits(xg_.buf), bits(xg_.before)) and torch.equal(bits(ssq_in.buf), bits(ssq_in.before)), f"{t2}: an input was written"
                        if first is None:
                            first = got.clone()
                        else:
                            assert torch.equal(bits(got), bits(first)), f"{t2}: differs from the first launch of this case (repeat, or blocked against row-major x)"
    report("exact")


HEAD = [(1, 64), (8, 96), (9, 64), (16, 96), (17, 64), (33, 96), (64, 64)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("B,K", HEAD, ids=[f"B{b}-K{k}" for b, k in HEAD])
def test_head_candidates_planted(ctx, dt, B, K):
    """N = 515, positive x: a NaN weight row (its logits are NaN and never chosen), a row block of NaN rows ((-inf, 0x7fffffff)), the three valid rows
    of the last block all negative (the zero-padded rows 515..527 would win if they were not excluded), one row block per workgroup (B <= 8) and
    eight with seven tiles past the matrix (B >= 9: the candidate arrays end right behind row block 32, and the guard zone behind them is as long
    as those seven tiles).  Logits bitwise float64; every launch twice, blocked against row-major x."""
    N, nrb = 515, 33
    wi = int_weights(N, K, W16, ties=True)[0].clone()
    wi[37], wi[64:80], wi[512:515] = NAN, NAN, -1.0
    x64 = int_x(K, positive=True)
    wt = Weights(ctx, wi, dt, W16)
    want = (x64[:B] @ torch.nan_to_num(wi, nan=0.0).t()).to(DEV)
    want[:, torch.isnan(wi[:, 0])] = NAN
    assert bool((want[:, 512:515] < 0).all())
    ct, amax_ts, ldo = col_tiles(B), 16 * nrb, N + 3
    first = None
    for blocked, rep in [(bl, rep) for bl in ([True, False] if xblk_tiles(B) else [False]) for rep in range(2)]:
        xg_, xp, ldx = x_operand(x64, B, K, dt, blocked)
        out, av, ai = Guarded(B * ldo, torch.float32, -5.0), Guarded(ct * amax_ts, torch.float32, NAN), Guarded(ct * amax_ts, torch.int32, -7)
        _, ran = gemv_ex(ctx, dt, F32, wt, xp, ldx, out.body, ldo, N, K, B, amax_val=av.body, amax_idx=ai.body, ssq_ts=16, amax_ts=amax_ts, x_blocked=blocked)
        tag = f"head planted B={B} K={K} {DTN[dt]} {'blocked' if blocked else 'row-major'} x launch {rep}"
        assert_shape(ran, (1 if B <= 8 else 8, ct, int(B <= 8), 0, 0, W16), tag)
        got = out.body.view(B, ldo)[:, :N]
        assert same_bits(got, want.float()), f"{tag}: logits differ from float64"
        out.expect(overlay(out, B, ldo, N, got), tag + " guards")
        check_candidates(av, ai, got, N, B, amax_ts, tag, need_tie=True)
        cand_v, cand_i = tiles_decode(av.body, nrb, ct, amax_ts)[:, :B], tiles_decode(ai.body, nrb, ct, amax_ts)[:, :B]
        assert bool((cand_v[4] == -math.inf).all()) and bool((cand_i[4] == NO_IDX).all()), f"{tag}: the all-NaN block"
        assert bool((cand_i[2] != 37).all()) and bool(torch.isfinite(cand_v[2]).all()), f"{tag}: the NaN logit of row 37"
        assert bool((cand_v[32] < 0).all()) and bool((cand_i[32] <= 514).all()), f"{tag}: a zero-padded row past N = 515 was chosen"
        if first is None:
            first = (got.clone(), cand_v.clone(), cand_i.clone())
        else:
            assert same_bits(got, first[0]) and torch.equal(bits(cand_v), bits(first[1])) and torch.equal(cand_i, first[2]), f"{tag}: differs from the first launch of this case (repeat, or blocked against row-major x)"


# --------------------------------------------------------------------------------------------------
# 1b. producers: 16-row and 8-phase forms
# --------------------------------------------------------------------------------------------------
# (format, N, K, Bs, dtypes, 8-phase row blocks per workgroup or 0)
PRODUCER16 = [(W16, n, k, BS, DTYPES, 0) for n in (16, 128, 1024) for k in KS] + \
             [(FP8, n, k, BS, DTYPES, 0) for n in (16, 128, 1024) for k in (64, 192)] + \
             [(W12, n, k, NARROW, [torch.bfloat16], 0) for n in (16, 128, 1024) for k in (64, 192)]
PRODUCER8 = [(W16, 128, 1024, [33, 48, 64], DTYPES, 8), (W16, 1024, 1024, [33, 64], DTYPES, 8), (W16, 256, 1056, [33, 64], DTYPES, 8),
             (W16, 128, 6208, [33, 64], DTYPES, 8), (W16, 128, 8192, [17, 32], DTYPES, 8), (W16, 5120, 1024, [33], DTYPES, 10),
             (FP8, 128, 1024, [48], DTYPES, 8), (FP8, 128, 12288, [1, 8, 9, 16], DTYPES, 8), (FP8, 5120, 4096, [8, 16], DTYPES, 10)]
PRODUCER_CASES = [(f, n, k, dt) for f, n, k, _, dts, _ in PRODUCER16 + PRODUCER8 for dt in dts]


def run_producer(ctx, dt, wt, x64, r_old, gamma, N, K, B, blocked, k8, tag, shape):
    """One producer launch on sentinel-guarded buffers: (residual, xg, ssq_out, k8_part) as Guarded and the layout facts (ldo, ssq_ts)."""
    ct, ldo, ssq_ts = col_tiles(B), N + 4, N + 16
    xg_in, xv = rows2d(x64[:B].to(DEV), K + 8, dt, NAN, extra_rows=1)
    res, _ = rows2d(r_old[:B].to(DEV), ldo, torch.float32, NAN, extra_rows=1)
    xg = Guarded(ct * 16 * N if blocked else (B + 1) * ldo, dt, NAN)
    ssq = Guarded(ct * ssq_ts, torch.float32, NAN)
    part = Guarded((N // 16) * 8 * ct * 256, torch.float32, NAN) if k8 else None
    _, ran = gemv_ex(ctx, dt, RESIDNORM, wt, xv, K + 8, res.body, ldo, N, K, B, gamma=gamma, xg=xg.body, ssq_out=ssq.body, ssq_ts=ssq_ts,
                     k8=part.body if part else None, x_blocked=blocked)
    assert_shape(ran, shape, tag)
    assert torch.equal(bits(xg_in.buf), bits(xg_in.before)), f"{tag}: x was written"
    assert part is None or part.guards_ok(), f"{tag}: the guard zones of k8_part were written"
    return res, xg, ssq, ldo, ssq_ts


@gpu
@pytest.mark.parametrize("fmt,N,K,dt", PRODUCER_CASES, ids=[f"{FMTN[f]}-{n}x{k}-{DTN[dt]}" for f, n, k, dt in PRODUCER_CASES])
def test_producer_exact(ctx, fmt, N, K, dt):
    """GV_RESIDNORM with integer inputs and power-of-two gamma: the new residual, xg = round16(r gamma) (row-major, and blocked where B > 8 and
    N % 32 == 0) and every ssq_out[ct][rb][b] (0 for b >= B) bitwise float64; residual, xg, ssq_out inside sentinel buffers compared as a whole
    (guard zones, pad columns, the xg slots of absent sequences), k8_part between guard zones; twice.  The 16-row form runs without k8_part, the
    8-phase cases name the mapping they select: N = 128 / 256 one or two row groups ((R & 7) != 0), N = 1024 / 5120 the XCD-grouped ids, 5120 ten row blocks per
    workgroup, K = 1056 the K % 64 == 32 staging, K = 6208 two passes for phase 0 at four column tiles."""
    _, _, _, Bs, _, nwb = next(c for c in PRODUCER16 + PRODUCER8 if c[:3] == (fmt, N, K))
    wi, rs = int_weights(N, K, fmt)
    x64, r_old = int_x(K), r_old_case(N)
    rnew = r_old + (x64 @ wi.t()) * rs
    check_exact(x64, wi, float(rs.min()), rnew)
    g = torch.Generator().manual_seed(N + K)
    gamma64 = torch.exp2(torch.randint(-3, 2, (N,), generator=g).double())
    gamma = gamma64.float().to(DEV)
    wt = Weights(ctx, wi * rs[:, None], dt, fmt)
    for B in Bs:
        ct = col_tiles(B)
        shape = (1, ct, 0 if nwb else int(B <= 8), int(nwb > 0), nwb, W12 if (fmt == W12 and ct == 1) else fmt)
        r = rnew[:B].to(DEV)
        want_xg = (r * gamma64.to(DEV)).to(dt)
        want_ssq = (r * r).view(B, N // 16, 16).sum(-1).t().contiguous().float()           # [N / 16, B]
        for blocked in ([True, False] if (xblk_tiles(B) and N % 32 == 0) else [False]):
            first = None
            for rep in range(2):
                tag = f"producer {FMTN[fmt]} N={N} K={K} B={B} {DTN[dt]} {'blocked' if blocked else 'row-major'} xg"
                res, xg, ssq, ldo, ssq_ts = run_producer(ctx, dt, wt, x64, r_old, gamma, N, K, B, blocked, nwb > 0, tag, shape)
                res.expect(overlay(res, B, ldo, N, r.float()), tag + " residual", locate=loc2d(ldo, "b"))
                if blocked:
                    xg.expect(xblk_encode(want_xg, ct, NAN), tag + " xg", locate=lambda i: f"k-block {i // (ct * 512)} tile {(i // 512) % ct} b {(i // 8) % 16}")
                else:
                    xg.expect(overlay(xg, B, ldo, N, want_xg), tag + " xg", locate=loc2d(ldo, "b"))
                ssq.expect(tiles_encode(want_ssq, ct, ssq_ts, 0.0, NAN), tag + " ssq_out", locate=lambda i: f"tile {i // ssq_ts} row block {(i % ssq_ts) // 16} b {i % 16}")
                if first is None:
                    first = (res.buf.clone(), xg.buf.clone(), ssq.buf.clone())
                else:
                    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, (res.buf, xg.buf, ssq.buf))), f"{tag}: the second launch differs"


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
def test_resid_exact(ctx, dt):
    """Mode 1 (fp32 out += y: the entry accepts it, a decode step runs the producer in its place) with integer inputs: the residual bitwise float64
    inside its sentinel buffer at every B, one row block per workgroup; blocked and row-major x give the same bits; every launch twice."""
    N, K, ldo = 48, 96, 52
    wi = int_weights(N, K, W16)[0]
    x64, r_old = int_x(K), r_old_case(N)
    check_exact(x64, wi)
    wt = Weights(ctx, wi, dt, W16)
    for B in BS:
        want = (r_old[:B] + x64[:B] @ wi.t()).to(DEV).float()
        for blocked, rep in [(bl, rep) for bl in ([True, False] if xblk_tiles(B) else [False]) for rep in range(2)]:
            tag = f"resid N={N} K={K} B={B} {DTN[dt]} {'blocked' if blocked else 'row-major'} x launch {rep}"
            xg_, xp, ldx = x_operand(x64, B, K, dt, blocked)
            res, _ = rows2d(r_old[:B].to(DEV), ldo, torch.float32, NAN, extra_rows=1)
            _, ran = gemv_ex(ctx, dt, RESID, wt, xp, ldx, res.body, ldo, N, K, B, x_blocked=blocked)
            assert_shape(ran, (1, col_tiles(B), int(B <= 8), 0, 0, W16), tag)
            res.expect(overlay(res, B, ldo, N, want), tag, locate=loc2d(ldo, "b"))
            assert torch.equal(bits(xg_.buf), bits(xg_.before)), f"{tag}: x was written"


@gpu
def test_prep_and_embed_exact(ctx):
    """embed_tok_norm_kernel and resid_norm_prep_kernel with integer rows and power-of-two gamma: resid (embed), xg row-major / blocked and the one
    partial per sequence at [b / 16][0][b % 16] with tile stride H, bitwise; everything else in the buffers keeps its bits; every launch twice."""
    for dt in DTYPES:
        for H in (32, 128, 1024, 2080):
            g = torch.Generator().manual_seed(H)
            table = torch.randint(-8, 9, (40, H), generator=g).double()
            gamma64 = torch.exp2(torch.randint(-3, 2, (H,), generator=g).double())
            gamma = gamma64.float().to(DEV)
            for B in BS:
                ct = col_tiles(B)
                tok = torch.randint(0, 40, (B,), generator=g)
                r = table[tok].to(DEV)
                assert float((r * r).sum(-1).max()) < 2 ** 24
                want_xg, want_ssq = (r * gamma64.to(DEV)).to(dt), (r * r).sum(-1)[None].float()
                for embed in (True, False):
                    for blocked in (True, False):
                        blk = blocked and xblk_tiles(B) > 0
                        tb, tk = table.to(dt).to(DEV), tok.to(torch.int32).to(DEV)
                        for rep in range(2):                     # fresh sentinel buffers each time: both launches are held to the same bits
                            res = Guarded(B * H, torch.float32, NAN, init=None if embed else r)
                            xg = Guarded(ct * 16 * H if blk else B * H, dt, NAN)
                            ssq = Guarded(ct * H, torch.float32, NAN)
                            gemv_prep(ctx, dt, tk if embed else None, tb if embed else None, res.body, gamma, xg.body, ssq.body, B, H, blocked)
                            tag = f"{'embed' if embed else 'prep'} H={H} B={B} {DTN[dt]} {'blocked' if blk else 'row-major'} launch {rep}"
                            res.expect(r.float(), tag + " resid")
                            xg.expect(xblk_encode(want_xg, ct, NAN) if blk else want_xg, tag + " xg")
                            ssq.expect(tiles_encode(want_ssq, ct, H, NAN, NAN), tag + " ssq")


@gpu
def test_gemv_ex_rejects_bad_arguments(ctx):
    """A wrong test argument is an error code, not a stray write: nothing is launched (the output keeps its NaN)."""
    from video_llava_amd import _lib
    dt, N, K, B = torch.float16, 64, 64, 33
    wt = Weights(ctx, int_weights(N, K, W16)[0], dt, W16)
    x, out = torch.zeros(64, K, dtype=dt, device=DEV), torch.full((64, N), NAN, dtype=torch.float32, device=DEV)
    f = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    gm, xg, so, av, ai = f(N), torch.zeros(64 * N, dtype=dt, device=DEV), f(4 * N), f(4 * 64), torch.zeros(4 * 64, dtype=torch.int32, device=DEV)
    good = dict(gamma=gm, xg=xg, ssq_out=so, ssq_ts=N, k8=f(N // 16 * 8 * 4 * 256))
    assert gemv_ex(ctx, dt, RESIDNORM, wt, x, K, out, N, N, K, B, **good)[0] == _lib.PGV_OK
    out.fill_(NAN)
    bad = [dict(good, ssq_ts=N - 16), dict(good, gamma=None), dict(good, xg=None), dict(good, ssq_out=None), dict(good, k8_bytes=N // 16 * 8 * 4 * 1024 - 1)]
    for kw in bad:
        assert gemv_ex(ctx, dt, RESIDNORM, wt, x, K, out, N, N, K, B, ok=False, **kw)[0] == _lib.PGV_EINVAL, kw.keys()
    for mode, kw in ((4, {}), (F32, dict(amax_val=av)), (F32, dict(amax_val=av, amax_idx=ai, amax_ts=48)), (STORE16, dict(amax_val=av, amax_idx=ai, amax_ts=64)),
                     (STORE16, dict(ssq_in=so, nparts=0, ssq_ts=64)), (STORE16, dict(ssq_in=so, nparts=8, hidden=128, ssq_ts=64)), (STORE16, dict(gamma=gm)),
                     (RESID, dict(ssq_in=so, nparts=1, hidden=128, ssq_ts=16)), (STORE16, dict(k8=so))):
        assert gemv_ex(ctx, dt, mode, wt, x, K, out, N, N, K, B, ok=False, **kw)[0] == _lib.PGV_EINVAL, (mode, kw.keys())
    assert gemv_ex(ctx, dt, STORE16, wt, x, K - 8, out, N, N, K, B, ok=False, x_blocked=False)[0] == _lib.PGV_EINVAL
    assert gemv_ex(ctx, dt, STORE16, wt, x, K, out, N - 4, N, K, B, ok=False)[0] == _lib.PGV_EINVAL
    assert gemv_ex(ctx, dt, STORE16, wt, x, K, out, N, N, K, 65, ok=False)[0] == _lib.PGV_EINVAL
    assert torch.isnan(out).all()
    assert gemv_prep(ctx, dt, None, None, out, gm, xg, so, 4, 48, True, ok=False) == _lib.PGV_EINVAL
    assert gemv_prep(ctx, dt, ai, None, out, gm, xg, so, 4, 64, True, ok=False) == _lib.PGV_EINVAL


# --------------------------------------------------------------------------------------------------
# 2. the chain on real inputs
# --------------------------------------------------------------------------------------------------
def operand_bound(r, Er, gamma, dt):
    """xg = round16(fl32(r gamma)): (reference, bound)."""
    x = r * gamma
    Ex = rnd(x, gamma.abs() * Er)
    return x, Ex + hulp(x.abs() + Ex, dt)


def acc_bound(x, Ex, W):
    """x W^T accumulated in fp32 from an operand known to Ex: (reference, bound)."""
    K = x.shape[1]
    Wa = W.abs().t()
    return x @ W.t(), Ex @ Wa + K * UACC * ((x.abs() + Ex) @ Wa)


def partial_bound(r, Er):
    """A producer's sums of 16 squares [B, N / 16]: (reference, bound)."""
    B = r.shape[0]
    mag = r.abs() + Er
    return (r * r).view(B, -1, 16).sum(-1), (2 * r.abs() * Er + Er * Er).view(B, -1, 16).sum(-1) + 6 * U32 * (mag * mag).view(B, -1, 16).sum(-1)


def rstd_from_parts(p, Ep, H):
    """The consumer's rstd from P partials [B, P] known to Ep."""
    P = p.shape[1]
    ss = p.sum(-1)
    return rstd_bound(ss, Ep.sum(-1) + (P - 1) * U32 * (p + Ep).sum(-1), H, EPS)


def test_chain_bounds_cover_fp32_arithmetic_and_reject_a_wrong_partial():
    """Host only.  A plain fp32 evaluation of producer -> consumer stays inside the chain's bounds; a consumer that skips one partial, or a
    producer that adds the projection twice, leaves them."""
    g = torch.Generator().manual_seed(9)
    for dt in DTYPES:
        B, H, K, N = 6, 128, 96, 48
        x = torch.randn(B, K, generator=g).to(dt).double()
        Wo = (torch.randn(H, K, generator=g) / K ** 0.5).to(dt).double()
        Wc = (torch.randn(N, H, generator=g) / H ** 0.5).to(dt).double()
        r0, gamma = torch.randn(B, H, generator=g).float().double(), (1 + 0.2 * torch.randn(H, generator=g)).float().double()
        y, Ey = acc_bound(x, torch.zeros_like(x), Wo)
        r, Er = r0 + y, rnd(r0 + y, Ey)
        xg, Exg = operand_bound(r, Er, gamma, dt)
        p, Ep = partial_bound(r, Er)
        rstd, Erstd = rstd_from_parts(p, Ep, H)
        acc, Eacc = acc_bound(xg, Exg, Wc)
        out, Eout = scaled_bound(acc, Eacc, rstd, Erstd)
        Eout = Eout + hulp(out.abs() + Eout, dt)
        assert float(((out - rms_norm_linear(r, gamma, Wc, EPS)).abs() / Eout).max()) < 0.05          # the model itself is exact
        r32 = r0.float() + x.float() @ Wo.float().t()
        xg32 = (r32 * gamma.float()).to(dt)
        p32 = (r32 * r32).view(B, -1, 16).sum(-1)
        rs32 = torch.rsqrt(p32.sum(-1) * torch.tensor(1.0 / H) + torch.tensor(EPS, dtype=torch.float32))
        o32 = ((xg32.float() @ Wc.float().t()) * rs32[:, None]).to(dt)
        assert ((r32.double() - r).abs() <= Er).all() and ((xg32.double() - xg).abs() <= Exg).all() and ((p32.double() - p).abs() <= Ep).all()
        assert ((rs32.double() - rstd).abs() <= Erstd).all() and ((o32.double() - out).abs() <= Eout).all()
        skipped = torch.rsqrt((p32.sum(-1) - p32[:, 3]) * torch.tensor(1.0 / H) + torch.tensor(EPS, dtype=torch.float32))
        assert ((skipped.double() - rstd).abs() > Erstd).all()
        twice = r32 + x.float() @ Wo.float().t()
        assert (((twice.double() - r).abs() > Er).double().mean()) > 0.9


CHAIN = [(B, H) for H in (128, 1024) for B in (3, 16, 40)]


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("B,H", CHAIN, ids=[f"B{b}-H{h}" for b, h in CHAIN])
def test_chain_vs_fp64(ctx, dt, B, H):
    """prep / embed -> qkv -> o_proj -> gate/up -> down_proj -> head on device buffers handed from stage to stage (xg blocked at B > 8), attention
    replaced by a given 16-bit operand.  Every element of every intermediate within its propagated bound of float64 RMSNorm -> Linear; the head's
    candidates against its stored logits.  H = 1024 at B = 40 runs both producers in the 8-phase form.  Every launch runs twice (a producer from
    the same old residual) and must leave the same bits in everything it writes."""
    from video_llava_amd import _lib
    g = torch.Generator().manual_seed(B * 7 + H)
    I, V, ct = 2 * H, 515, col_tiles(B)
    blocked = xblk_tiles(B) > 0

    def w16(n, k, s=1.0):
        return (torch.randn(n, k, generator=g) * s / k ** 0.5).to(dt).double()
    Wqkv, Wo, Wgu, Wd, Wh = w16(3 * H, H), w16(H, H), w16(2 * I, H), w16(H, I), w16(V, H, 2.0)
    gam = [(1 + 0.2 * torch.randn(H, generator=g)).float().double() for _ in range(3)]
    table = torch.randn(48, H, generator=g).to(dt).double() * 2
    tok = torch.randint(0, 48, (B,), generator=g)
    ao = torch.randn(B, H, generator=g).to(dt).double()
    use_embed = B != 16
    r0 = table[tok] if use_embed else (torch.randn(B, H, generator=g) * 2).float().double()
    dev = lambda t: t.to(DEV)
    wts = {k: Weights(ctx, w, dt, W16) for k, w in (("qkv", Wqkv), ("o", Wo), ("gu", Wgu), ("d", Wd), ("h", Wh))}
    key = lambda s: (f"chain {s}", DTN[dt])
    tag = f"chain B={B} H={H} {DTN[dt]}"
    n_xg = ct * 16 * H if blocked else B * H
    loc = loc2d

    def xg_rows(buf):
        return (xblk_decode(buf, H, ct) if blocked else buf.view(B, H))[:B]

    # stage 0: prep / embed
    resid = Guarded(B * H, torch.float32, NAN, init=None if use_embed else dev(r0))
    xg, ssq = Guarded(n_xg, dt, 0.0), Guarded(ct * H, torch.float32, 0.0)
    tb, tk, g0 = dev(table).to(dt), dev(tok).to(torch.int32), dev(gam[0]).float()
    once = None
    for rep in range(2):                                           # twice: the same bits
        gemv_prep(ctx, dt, tk if use_embed else None, tb if use_embed else None, resid.body, g0, xg.body, ssq.body, B, H, True)
        now = [resid.buf.clone(), xg.buf.clone(), ssq.buf.clone()]
        assert once is None or all(torch.equal(bits(a), bits(b)) for a, b in zip(once, now)), f"{tag}: the second launch of the first stage differs"
        once = now
    r, Er = dev(r0), torch.zeros(B, H, dtype=torch.float64, device=DEV)
    assert torch.equal(resid.body.view(B, H).double(), r), f"{tag}: the residual of the first stage is exact"
    x, Ex = operand_bound(r, Er, dev(gam[0]), dt)
    assert_bound(xg_rows(xg.body), x, Ex, tag + " xg0", key("prep xg"), loc(H, "b"))
    p = (r * r).sum(-1, keepdim=True)
    Ep = H * U32 * p
    assert_bound(tiles_decode(ssq.body, 1, ct, H)[:, :B].t(), p, Ep, tag + " ssq0", key("prep ssq"), loc(1, "b"))
    rstd, Erstd = rstd_from_parts(p, Ep, H)

    def consumer(mode, name, W, gamma, N, nparts, tl_n, tl_w, amax=False):
        No, odt = (N // 2 if mode == SWIGLU else N), (torch.float32 if mode == F32 else dt)
        out = Guarded(B * No, odt, NAN)
        nrb = (N + 15) // 16
        av, ai = (Guarded(ct * 16 * nrb, torch.float32, NAN), Guarded(ct * 16 * nrb, torch.int32, -7)) if amax else (None, None)
        tl = tl_w if B > 16 else tl_n[B > 8]
        once = None
        for rep in range(2):                                       # every launch twice: the same bits in every output
            for gd in (out, av, ai):
                if gd is not None:
                    gd.buf.copy_(gd.before)
            _, ran = gemv_ex(ctx, dt, mode, wts[name], xg.body, H, out.body, No, N, H, B, ssq_in=ssq.body, nparts=nparts, hidden=H, eps=EPS, ssq_ts=H,
                             amax_val=av.body if amax else None, amax_idx=ai.body if amax else None, amax_ts=16 * nrb)
            assert_shape(ran, (tl, ct, int(B <= 8), 0, 0, W16), f"{tag} {name}")
            now = [gd.buf.clone() for gd in (out, av, ai) if gd is not None]
            assert once is None or all(torch.equal(bits(a), bits(b)) for a, b in zip(once, now)), f"{tag} {name}: the second launch differs"
            once = now
        acc, Eacc = acc_bound(x, Ex, dev(W))
        y, Ey = scaled_bound(acc, Eacc, rstd, Erstd)
        hf = rms_norm_linear(r, dev(gamma), dev(W), EPS)           # HF's order of operations: the reference (equal to y up to float64 rounding)
        assert float((hf - y).abs().max()) <= 1e-12 * float(hf.abs().max())
        y = hf
        if mode == SWIGLU:
            y, Ey = swiglu_cols(y, Ey)
        if odt != torch.float32:
            Ey = Ey + hulp(y.abs() + Ey, dt)
        got = out.body.view(B, No)
        assert out.guards_ok(), f"{tag} {name}: guard zones"
        assert_bound(got, y, Ey, f"{tag} {name}", key(name), loc(No, "b"))
        if amax:
            check_candidates(av, ai, got, N, B, 16 * nrb, f"{tag} {name}")
        return out, y, Ey

    def producer(name, W, xin, xref, Exin, K, gamma):
        nonlocal r, Er
        k8 = Guarded((H // 16) * 8 * ct * 256, torch.float32, NAN)
        is8 = B > 32 and K // 64 >= 16 and (H // 16) % 8 == 0
        r_before, once = resid.buf.clone(), None
        for rep in range(2):                                       # every launch twice, from the same old residual: the same bits in residual, xg and ssq
            resid.buf.copy_(r_before)
            _, ran = gemv_ex(ctx, dt, RESIDNORM, wts[name], xin, K, resid.body, H, H, K, B, gamma=dev(gamma).float(), xg=xg.body, ssq_out=ssq.body, ssq_ts=H, k8=k8.body)
            assert_shape(ran, (1, ct, 0 if is8 else int(B <= 8), int(is8), 8 if is8 else 0, W16), f"{tag} {name}")
            now = [resid.buf.clone(), xg.buf.clone(), ssq.buf.clone()]
            assert once is None or all(torch.equal(bits(a), bits(b)) for a, b in zip(once, now)), f"{tag} {name}: the second launch differs"
            once = now
        assert k8.guards_ok() and resid.guards_ok() and xg.guards_ok() and ssq.guards_ok(), f"{tag} {name}: guard zones"
        y, Ey = acc_bound(xref, Exin, dev(W))
        r, Er = r + y, rnd(r + y, Er + Ey)
        assert_bound(resid.body.view(B, H), r, Er, f"{tag} {name} residual", key(name + " resid"), loc(H, "b"))
        xo, Exo = operand_bound(r, Er, dev(gamma), dt)
        assert_bound(xg_rows(xg.body), xo, Exo, f"{tag} {name} xg", key(name + " xg"), loc(H, "b"))
        pp, Epp = partial_bound(r, Er)
        got = tiles_decode(ssq.body, H // 16, ct, H)
        assert_bound(got[:, :B].t(), pp, Epp, f"{tag} {name} ssq", key(name + " ssq"), loc(H // 16, "b"))
        assert bool((got[:, B:] == 0).all()), f"{tag} {name}: the partials of absent sequences are 0"
        return xo, Exo, pp, Epp

    # the narrow store16 shapes at H = 1024: 192 row blocks -> tl 1 (64 workgroups of three are fewer than half the CUs)
    consumer(STORE16, "qkv", Wqkv, gam[0], 3 * H, 1, (1, 1), 3)
    aod = dev(ao).to(dt)
    x, Ex, p, Ep = producer("o", Wo, aod, dev(ao), torch.zeros(B, H, dtype=torch.float64, device=DEV), H, gam[1])
    rstd, Erstd = rstd_from_parts(p, Ep, H)
    act, a_ref, Ea = consumer(SWIGLU, "gu", Wgu, gam[1], 2 * I, H // 16, (2, 2), 4)
    x, Ex, p, Ep = producer("d", Wd, act.body, a_ref, Ea, I, gam[2])
    rstd, Erstd = rstd_from_parts(p, Ep, H)
    consumer(F32, "h", Wh, gam[2], V, H // 16, (1, 8), 8, amax=True)
    report("chain")
