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
