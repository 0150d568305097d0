"""Error-bound helpers shared by the element-wise kernel tests (test_gpu_gemm.py, test_gpu_gemv.py): device-agnostic float64 tensor arithmetic.
With u = 2^-24 (one fp32 rounding) rnd(x, E) = E + u (|x| + E) is the bound after one more rounding of a value x known to E."""
import numpy as np
import torch

U32 = 2.0 ** -24                                  # one fp32 rounding
UACC = 2.0 ** -23                                 # per addition of the MFMA accumulation
ULP1 = 2.0 ** -23                                 # "1 ulp" of v_exp_f32 / v_rcp_f32, relative
MINN = 2.0 ** -126                                # ... which return 0 where the result would be an fp32 denormal
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
K_SILU = float(np.float32(-1.4426950408889634))
EPS = float(np.float32(1e-5))


# --------------------------------------------------------------------------------------------------
# bounds (device-agnostic float64 tensor arithmetic)
# --------------------------------------------------------------------------------------------------
def rnd(x, E):
    """Error bound after one fp32 rounding of a value x known to E."""
    return E + U32 * (x.abs() + E)


def hulp(x, dt):
    """Half an ulp of `dt` at magnitude x."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** EMIN[dt]))
    return torch.ldexp(torch.ones_like(x), e - 2 - MANT[dt])


def sigmoid_mul_bound(x, E, k):
    """y = x * rcp(1 + exp2(x * k)) as the kernel evaluates it; returns (y exact with the real constant, bound)."""
    z = x * k
    Ez = rnd(z, abs(k) * E)
    t = torch.exp2(z)
    thi = t * torch.exp2(Ez)
    Et = (thi - t) + ULP1 * thi + MINN
    s = 1.0 + t
    Es = rnd(s, Et)
    r = 1.0 / s
    Er = Es / (s * (s - Es))
    Er = Er + ULP1 * (r + Er) + MINN
    y = x * r
    return y, rnd(y, x.abs() * Er + r * E + E * Er)


def silu_ref(x):
    return x / (1.0 + torch.exp(-x))


def swiglu_bound(g, Eg, u, Eu):
    y, Ey = sigmoid_mul_bound(g, Eg, K_SILU)
    Ey = Ey + (y - silu_ref(g)).abs()
    out = silu_ref(g) * u
    return rnd(out, u.abs() * Ey + silu_ref(g).abs() * Eu + Ey * Eu)


# --------------------------------------------------------------------------------------------------
# 16-bit rounding and the row norms of csrc/elementwise.hip (tests/test_gpu_frontend.py)
# --------------------------------------------------------------------------------------------------
def round16(x, dt):
    """The value of `dt` nearest to the float64 x (ties to even, subnormal spacing below 2^EMIN), as float64: ONE rounding, where torch's
    double -> 16-bit conversion rounds to fp32 first."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** EMIN[dt]))
    q = torch.ldexp(torch.ones_like(x), e - 1 - MANT[dt])
    return torch.round(x / q) * q


def midpoint_distance(x, dt):
    """Distance from the float64 x to the nearer of the two rounding midpoints of `dt` around round16(x)."""
    a, ra = x.abs(), round16(x, dt).abs()
    m, e = torch.frexp(ra.clamp_min(2.0 ** EMIN[dt]))
    up = torch.ldexp(torch.ones_like(x), e - 1 - MANT[dt])                 # spacing above |r|
    dn = torch.where((m == 0.5) & (e - 1 > EMIN[dt]), up / 2, up)          # ... and below it: half of that at a power of two
    return torch.minimum((a - (ra + up / 2)).abs(), (a - (ra - dn / 2)).abs())


def row_norm_bound(x, Ex, gamma, beta, eps, NV, rms=False):
    """norm_kernel / embed_ln_kernel on rows x [R, n] (n = 256 NV) known to Ex, fp32 gamma / beta [n]: (exact float64 result, bound of the
    fp32 result BEFORE any 16-bit rounding).  Every sum is taken in an order of depth <= NV + 8 (lane sums, then a 64-lane butterfly):
      mean   S^ - S <= (NV + 8) u sum|x|, times fl(1/n): two more roundings                                              -> Emu
      d_i    fl(x_i - mean^): Ex_i + Emu + one rounding                                                                  -> Ed
      ss     sum (x^_i - mean^)^2 = n var + n (mean - mean^)^2 + sum 2 e_i (x_i - mean^) + sum e_i^2 (the first-order term of the mean's error
             cancels), each term 2 u for d_i's rounding, u for the square, 4 NV + 5 additions deep; var = ss fl(1/n) (2 roundings), + eps (1)
      rstd   rsqrtf of that interval, 2 ulp
      out    fl(fl(fl(d rstd) gamma) + beta): a contraction to an FMA only removes a rounding.
    RMSNorm: mean = 0 exactly, no subtraction."""
    n = x.shape[-1]
    if rms:
        mu, Emu = torch.zeros_like(x[:, :1]), torch.zeros_like(x[:, :1])
        d, Ed = x, Ex
    else:
        mu = x.mean(-1, keepdim=True)
        Es = Ex.sum(-1, keepdim=True) + (NV + 8) * U32 * (x.abs() + Ex).sum(-1, keepdim=True)
        Emu = Es / n + 2 * U32 * (mu.abs() + Es / n)
        d = x - mu
        Ed = rnd(d, Ex + Emu)
    mag = d.abs() + Ex + Emu
    var = (d * d).mean(-1, keepdim=True)
    Ess = n * Emu * Emu + (2 * (d.abs() + Emu) * Ex + Ex * Ex).sum(-1, keepdim=True) + (4 * NV + 9) * U32 * (mag * mag).sum(-1, keepdim=True)
    Evar = Ess / n + 2 * U32 * (var + Ess / n)
    v = var + eps
    Ev = rnd(v, Evar)
    rstd = v ** -0.5
    Er = (v - Ev).clamp_min(1e-300) ** -0.5 - rstd
    Er = Er + 2 * ULP1 * (rstd + Er)
    p1 = d * rstd
    E1 = rnd(p1, d.abs() * Er + rstd * Ed + Ed * Er)
    t = p1 * gamma
    E2 = rnd(t, gamma.abs() * E1)
    out = t + beta
    return out, rnd(out, E2)
