"""GPU: the production residual producer (pgv_gemv_ex, mode 5: fp32 residual += W x, xg = round16(residual gamma), ssq_out) streams the 12-bit copy
through a register pipeline whose depth is a constant of its own (csrc/gemv.hip, kW12ProducerPU = D groups of 64 columns per buffer against the 2
of the 16-bit kernel; depths 1 to 4 were measured, 1 kept: LAB.md "12-bit producers: pipeline depth").  The arithmetic must not notice the depth or the format: the same launch with
the 16-bit matrix alone and with the 12-bit copy as well gives bitwise equal residual, xg and ssq_out.  (Run against a variant library of another
depth, every case still has to pass; the group counts below are the edge cases of depth D.)  N = 32 (two workgroups), bf16, B in {1, 8, 16} (the
merged x load and the two-load form), K = 64 G with the group counts at which a pipeline of depth D takes another path -- wave w of the eight
holds the groups w, w + 8, ..., in batches of D:
    G = 1          seven waves hold no group
    G = 8 D        exactly one full batch per wave
    G = 8 D + 1    one wave alone opens a second batch; the others' last batch is entirely past the end
    G = 16 D       two batches (the tail after a loop that is never entered)
    G = 16 D + 1   three batches, loop entered once
    G = 64, 172    the o_proj and down_proj shapes of the 7B decoder (172: waves with 22 and 21 groups)
Groups past the end re-read the last group against a zeroed x fragment, so every weight is finite (Inf / NaN placement is the business of the
encoder's adversarial test); exceptions (exponents outside the row window) sit in the first unit, in the last unit -- the one that is re-read --
and in the last group of a middle wave."""
import ctypes

import numpy as np
import pytest
import torch

import w12_numpy as w12

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 1                                              # kW12ProducerPU of csrc/gemv.hip
N = 32
GROUPS = [1, 8 * D, 8 * D + 1, 16 * D, 16 * D + 1, 64, 172]
RESIDNORM, WF_16, WF_12 = 5, 0, 2


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


@pytest.fixture(scope="module", params=GROUPS, ids=[f"G{g}" for g in GROUPS])
def case(request, ctx):
    """One matrix per group count: blocked 16-bit copy, 12-bit copy, activations, old residual, gamma -- built once, never written."""
    from video_llava_amd import _lib
    G = request.param
    K = 64 * G
    g = torch.Generator().manual_seed(1000 + G)
    bits = w12.bf16_bits((torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)).copy()
    bits[0, 0] = 0x0001; bits[0, 63] = 0x2F00                        # first unit
    bits[N - 1, K - 1] = 0x8001; bits[N // 2, K - 33] = 0x0000         # last unit (the group that is re-read past the end)
    mid = [j for j in range(G) if j % 8 == 4]                        # the groups of wave 4
    if mid:
        bits[N // 2, mid[-1] * 64 + 7] = 0x4480; bits[N // 2 + 1, mid[-1] * 64 + 40] = 0x0000
    w = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    assert torch.isfinite(w.float()).all()
    dc = _lib.dtype_code(torch.bfloat16)
    wb = torch.zeros(N * K, dtype=torch.bfloat16, device=DEV)
    _lib.check(ctx.lib.pgv_pack_blocked(ctx.handle, dc, w.to(DEV).contiguous().data_ptr(), N, K, wb.data_ptr(), _lib.stream_ptr()))
    buf = torch.zeros(int(ctx.lib.pgv_w12_bytes(N, K)), dtype=torch.uint8, device=DEV)
    counts = torch.zeros(N // 16, dtype=torch.int32, device=DEV)
    _lib.check(ctx.lib.pgv_encode_w12_blocked(ctx.handle, dc, wb.data_ptr(), buf.data_ptr(), counts.data_ptr(), N, K, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(counts.max()) <= 64 and int(counts[0]) >= 2 and int(counts[-1]) >= 1
    x = torch.randn(16, K, generator=g).to(torch.bfloat16).to(DEV)
    resid = torch.randn(16, N, generator=g).to(DEV)
    gamma = (1 + 0.2 * torch.randn(N, generator=g)).to(DEV)
    return G, K, wb, buf, x, resid, gamma


def _produce(ctx, K, B, wb, buf, x, resid, gamma):
    from video_llava_amd import _lib
    out = resid[:B].clone()
    xg = torch.full((B, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ssq = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    xb = x[:B].contiguous()
    d, sh = _lib.GemvDesc(), _lib.GemvShape(-1, -1, -1, -1, -1, -1)
    d.mode, d.d_W, d.d_W12 = RESIDNORM, wb.data_ptr(), (buf.data_ptr() if buf is not None else None)
    d.d_x, d.ldx, d.d_out, d.ldo, d.N, d.K, d.B = xb.data_ptr(), K, out.data_ptr(), N, N, K, B
    d.hidden, d.d_gamma, d.d_xg, d.d_ssq_out, d.ssq_ts = N, gamma.data_ptr(), xg.data_ptr(), ssq.data_ptr(), N
    d.d_k8_part, d.k8_part_bytes, d.x_blocked, d.shape = None, 0, 0, ctypes.pointer(sh)
    _lib.check(ctx.lib.pgv_gemv_ex(ctx.handle, _lib.dtype_code(torch.bfloat16), ctypes.byref(d), _lib.stream_ptr()), "pgv_gemv_ex")
    torch.cuda.synchronize()
    return out, xg, ssq, sh


@pytest.mark.parametrize("B", [1, 8, 16])
def test_w12_producer_bitwise_equals_16bit(ctx, case, B):
    G, K, wb, buf, x, resid, gamma = case
    r16, xg16, ssq16, sh16 = _produce(ctx, K, B, wb, None, x, resid, gamma)
    r12, xg12, ssq12, sh12 = _produce(ctx, K, B, wb, buf, x, resid, gamma)
    assert (sh16.wfmt, sh16.tl, sh16.k8) == (WF_16, 1, 0)
    assert sh12.wfmt == WF_12 and sh12.tl == 1 and sh12.k8 == 0
    assert torch.isfinite(r16).all() and not torch.equal(r16, resid[:B]), "the 16-bit launch did not run"
    assert torch.equal(_bits(r12), _bits(r16)), f"G = {G}, B = {B}: residual differs in {int((_bits(r12) != _bits(r16)).sum())} elements"
    assert torch.equal(_bits(xg12), _bits(xg16)), f"G = {G}, B = {B}: xg differs"
    assert torch.equal(_bits(ssq12), _bits(ssq16)), f"G = {G}, B = {B}: ssq_out differs"
    assert torch.isfinite(xg16.float()).all() and torch.isfinite(ssq16).all()
