"""GPU: the two LLaMA attention kernels of the decoder, called directly through their building blocks (pgv_decode_attention,
pgv_prefill_attention) and checked element by element against a float64 reference of the same operation.

Reference.  RoPE uses the product's table, built as HF's LlamaRotaryEmbedding builds it (fp32 inv_freq, fp32 angle, fp32 cos/sin; the cos/sin
come from the C library the product calls, so the table is the same bit for bit).  q and k are rotated in float64 and rounded once to the dtype;
scores use 128^-0.5, then an exact softmax and PV.  Decode attends to cache rows [0, pos) plus the fresh key at pos; prefill row i of a sequence
attends to keys [0, koff + i].

Bound, per output element: |out - ref| <= ulp_dtype(ref) + (gamma + expm1(2 Delta)) * sum_i p_i |v_i| / sum_i p_i  (+ a subnormal term, prefill fp16)
  ulp_dtype(ref)  the final rounding of the fp32 result to the dtype (half an ulp) with as much again for everything below.
  Delta           a bound on the error of every score (natural-log units): a perturbation |ds_i| <= Delta moves every softmax weight
                  p_i / sum p by a factor within [e^-2Delta, e^2Delta], so the output by at most expm1(2 Delta) * sum p|v| / sum p.
                  fp32 score arithmetic: decode sums 8 products per lane, then 4 DPP levels, and pre-scales q by a rounded scale*log2(e):
                  <= 16 u32 * S_abs, S_abs = 128^-0.5 * sum_e |q_e k_e|; prefill accumulates the 128 products in 8 chained MFMAs: 32 u32 * S_abs.
                  Decode also carries the rounding of its own rotated q and fresh k, which this reference cannot see: where the float64 value lies
                  within w = 2^-21 (|x1 c| + |x2 s|) of a rounding midpoint of the dtype (w bounds the kernel's fp32 rotation error, so it may round
                  either way) the element may be off by err = ulp + w (more than an ulp only where x1 c and x2 s nearly cancel), worth
                  128^-0.5 * err(q_e) |k_e| of score.  Everywhere else the kernel must write exactly the rounded value.
                  Prefill needs no such term: its rotated q and k are written back, checked, and fed to the reference.
  gamma           the fp32 weight arithmetic: v_exp_f32, the online rescales and the fp32 PV sums, about one rounding per 16 keys and per
                  merge level: (n / 8 + 64) u32 for n keys (an fp32-sized constant).  Prefill rounds P to the dtype before the PV MFMA
                  (the normaliser is summed from the unrounded values): one more u_dtype.  fp16 P below 2^-14 is subnormal: absolute error
                  2^-25 per key, hence + 2^-25 * sum_visible |v| / sum p.
The inputs make the bound bite: every decode unit (sequence, head) has one spike key carrying most of the softmax mass, at a position chosen per
unit so that the case covers 0, pos - 1, the fresh key, +-1 around 16/32/64/256-key boundaries and every 16-key group of a 4096-key context;
prefill uses large-norm q / k (score std 5) so rows are sharply peaked.  Negative controls evaluate the same bound against broken references
(fresh key dropped, last cached key dropped, masked row leaked, q rotated at pos +- 1, one 16-key group removed) and require each to fail it.
Rows of the cache past the valid range hold NaN / Inf in one variant and dominating finite keys with large v in the other: the outputs must be
bitwise the same.
"""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HD = 128
SCALE = HD ** -0.5
U32 = 2.0 ** -24
MAX_POS = 4096
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


# --------------------------------------------------------------------------------------------------
# reference helpers
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def rope_table():
    """cos / sin [MAX_POS + 2, 64] as float64 holding the fp32 values of the product's table, for positions -1 .. MAX_POS (row p + 1)."""
    libm = C.CDLL("libm.so.6")
    for fn in ("powf", "cosf", "sinf"):
        getattr(libm, fn).restype = C.c_float
    libm.powf.argtypes = [C.c_float, C.c_float]
    libm.cosf.argtypes = libm.sinf.argtypes = [C.c_float]
    inv = np.array([np.float32(1.0) / np.float32(libm.powf(10000.0, float(np.float32(2 * j) / np.float32(HD)))) for j in range(64)], np.float32)
    ang = np.arange(-1, MAX_POS + 1, dtype=np.float32)[:, None] * inv[None, :]          # fp32 products
    cos = np.vectorize(libm.cosf, otypes=[np.float64])(ang)
    sin = np.vectorize(libm.sinf, otypes=[np.float64])(ang)
    return torch.from_numpy(cos), torch.from_numpy(sin)


def ulp(x: torch.Tensor, dt) -> torch.Tensor:
    """Spacing of `dt` at |x| (float64)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** EMIN[dt]))
    return torch.ldexp(torch.ones_like(x), e - 1 - MANT[dt])


def round_to(x: torch.Tensor, dt) -> torch.Tensor:
    return x.float().to(dt).double()


def rotate(x: torch.Tensor, pos: torch.Tensor, dt):
    """Rotate-half RoPE of x [..., 128] (dtype values) at integer positions `pos` (broadcast over x's leading dims) in float64.
    Returns (rounded rotation, per-element allowance for the kernel's fp32 rotation: 0 where its rounding is unambiguous, else one ulp plus
    the fp32 error bound -- more than an ulp where x1 c and x2 s nearly cancel)."""
    cos, sin = rope_table()
    c, s = cos[pos + 1], sin[pos + 1]
    x = x.double()
    x1, x2 = x[..., :64], x[..., 64:]
    r = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    w = 2.0 ** -21 * torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    r16 = round_to(r, dt)
    amb = round_to(r + w, dt) != round_to(r - w, dt)
    return r16, amb * (ulp(r16, dt) + w)


def softmax_pv(s: torch.Tensor, v: torch.Tensor, mask: torch.Tensor | None = None):
    """s [..., R, n] natural-log scores of R queries, v [..., n, 128]: (sum p v / sum p, sum p |v| / sum p, p / max, sum p)."""
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    return p @ v / den, p @ v.abs() / den, p, den


def bound_fails(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    return ~((out - ref).abs() <= bound)          # NaN fails


def assert_within(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str):
    bad = bound_fails(out, ref, bound)
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        n = int(bad.sum())
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside the bound; first at {idx}: out {float(out[tuple(idx)])!r} "
                             f"ref {float(ref[tuple(idx)])!r} bound {float(bound[tuple(idx)]):.3e}")


def assert_rotation(got: torch.Tensor, ref: torch.Tensor, err: torch.Tensor, dt, what: str):
    """The kernel's rounded rotation: exactly the rounded float64 value where err == 0, else within max(1 ulp, err)."""
    bad = ((got - ref).abs() > torch.maximum(ulp(ref, dt), err)) | ((err == 0) & (got != ref))
    if bad.any():
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off; first at {list(idx)}: kernel {float(got[idx])!r} "
                             f"float64 rounded {float(ref[idx])!r} allowance {float(err[idx]):.3e}")


# --------------------------------------------------------------------------------------------------
# library handles and launches
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(ctx):
    """One weightless 1-layer model per (dtype, heads): the entries only take its dtype, head count and RoPE table."""
    from video_llava_amd import _lib
    made = {}
    for dt in (torch.float16, torch.bfloat16):
        for heads in (32, 40):
            cfg = _lib.LlmConfig(vocab=64, hidden=heads * HD, inter=11008 if heads == 32 else 13824, layers=1, heads=heads, eps=1e-5, rope_theta=10000.0)
            h = C.c_void_p()
            _lib.check(ctx.lib.pgv_llm_create(ctx.handle, C.byref(cfg), _lib.dtype_code(dt), C.byref(h)), "pgv_llm_create")
            made[(dt, heads)] = h
    yield made
    for h in made.values():
        ctx.lib.pgv_llm_destroy(h)


def ints(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def decode_call(ctx, llm, qkv, pos, K, V, out, max_seq, split, part, ticket):
    from video_llava_amd import _lib
    return ctx.lib.pgv_decode_attention(ctx.handle, llm, qkv.data_ptr(), ints(pos), K.data_ptr(), V.data_ptr(), out.data_ptr(), len(pos), max_seq,
                                        split, part.data_ptr(), ticket.data_ptr(), _lib.stream_ptr())


def prefill_call(ctx, llm, qkv, lens, koff, K, V, out, max_seq):
    from video_llava_amd import _lib
    return ctx.lib.pgv_prefill_attention(ctx.handle, llm, qkv.data_ptr(), ints(lens), ints(koff) if koff is not None else None, K.data_ptr(),
                                         V.data_ptr(), out.data_ptr(), len(lens), max_seq, _lib.stream_ptr())


def nan_poison(shape, dt):
    """NaN, +Inf, -Inf repeating along the last dimension."""
    pat = torch.tensor([math.nan, math.inf, -math.inf], dtype=torch.float32, device=DEV)
    return pat[torch.arange(shape[-1], device=DEV) % 3].to(dt).expand(shape)


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(torch.int16)


# --------------------------------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------------------------------
RAGGED = [0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 4094, 4095]
DECODE_CASES = {
    # name: (positions, max_seq, spike placement)
    "ragged": (RAGGED, 4096, "boundaries"),
    "groups4096": ([4064, 4079, 4080, 4081, 4090, 4093, 4094, 4095], 4096, "groups"),
    "max_seq77": ([76, 76, 75, 64, 63, 33, 16, 1], 77, "boundaries"),
    "b1": ([3000], 4096, "boundaries"),
    "b17": ([599, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 400, 512], 600, "boundaries"),
    "b64": ([(37 * i) % 300 for i in range(61)] + [0, 298, 299], 300, "boundaries"),
}


def spike_positions(pos, heads, mode):
    """Spike key of every unit (b, h): index in [0, pos] (pos = the fresh key)."""
    t = np.zeros((len(pos), heads), np.int64)
    for b, p in enumerate(pos):
        if mode == "groups":                  # unit u's spike in 16-key group u (mod 256): every group of a 4096-key context is covered
            for h in range(heads):
                u = b * heads + h
                t[b, h] = min(16 * (u % 256) + (3 * u) % 16, p)
            continue
        cand = [p, p - 1, 0]
        for m in (16, 32, 48, 64, 128, 192, 256, 512, 1024, 2048, 4096):
            cand += [m - 1, m, m + 1]
        seen, cs = set(), []
        for x in cand:
            if 0 <= x <= p and x not in seen:
                seen.add(x)
                cs.append(x)
        for h in range(heads):
            t[b, h] = cs[(h + b) % len(cs)] if h >= 3 else cs[h % len(cs)]
    return t


@functools.lru_cache(maxsize=1)
def decode_case(name, dt, heads):
    """Inputs (on the device) and the float64 reference of one decode case; asserts the negative controls."""
    pos, max_seq, mode = DECODE_CASES[name]
    B, H = len(pos), heads * HD
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(f'{name}/{heads}/{MANT[dt]}'.encode()))
    qkv = torch.randn(B, 3 * H, generator=g, device=DEV).to(dt)
    K = torch.randn(B, heads, max_seq, HD, generator=g, device=DEV).to(dt)
    V = torch.randn(B, heads, max_seq, HD, generator=g, device=DEV).to(dt)
    tpos = torch.tensor(pos, dtype=torch.long)
    q = qkv[:, :H].view(B, heads, HD).cpu()
    qrot, qamb = rotate(q, tpos[:, None], dt)                             # [B, heads, 128]
    # spikes: a key along the rotated q whose score is ln(n) + 2 (about 80 % of the mass)
    spike = spike_positions(pos, heads, mode)
    n = tpos + 1
    target = (torch.log(n.double()) + 2.0)[:, None, None]
    kspike = round_to(qrot * target / (SCALE * (qrot * qrot).sum(-1, keepdim=True)), dt)     # rotated-key space
    kraw = qkv[:, H:2 * H].view(B, heads, HD).cpu().double()
    cached = torch.from_numpy(spike) < tpos[:, None]
    bi, hi = cached.nonzero(as_tuple=True)
    K[bi.to(DEV), hi.to(DEV), torch.from_numpy(spike)[bi, hi].to(DEV)] = kspike[bi, hi].to(dt).to(DEV)
    cos, sin = rope_table()
    c, s = cos[tpos + 1][:, None], sin[tpos + 1][:, None]
    y1, y2 = kspike[..., :64], kspike[..., 64:]
    kraw = torch.where(cached[..., None], kraw, torch.cat([y1 * c + y2 * s, y2 * c - y1 * s], -1))    # fresh spikes: un-rotated, the kernel rotates back
    qkv[:, H:2 * H] = kraw.to(dt).reshape(B, H).to(DEV)
    kfresh, kamb = rotate(qkv[:, H:2 * H].view(B, heads, HD).cpu(), tpos[:, None], dt)
    vfresh = qkv[:, 2 * H:].view(B, heads, HD).cpu().double()
    rows = torch.arange(max_seq, device=DEV)[None, None, :, None] >= torch.tensor(pos, device=DEV)[:, None, None, None]   # [B, 1, max_seq, 1]
    K = torch.where(rows, nan_poison(K.shape, dt), K)
    V = torch.where(rows, nan_poison(V.shape, dt), V)
    # the dominating variant: keys along the rotated q with score 60, v = +-1e4
    kdom = round_to(qrot * (60.0 / (SCALE * (qrot * qrot).sum(-1, keepdim=True))), dt).to(dt).to(DEV)[:, :, None, :].expand_as(K)
    vdom = (1e4 * (1 - 2 * (torch.arange(HD, device=DEV) % 2))).to(dt).expand_as(V)

    ref = torch.empty(B, heads, HD, dtype=torch.float64)
    bound = torch.empty_like(ref)
    fails = {k: False for k in ("fresh key dropped", "last cached key dropped", "q rotated at pos + 1", "q rotated at pos - 1")}
    spike_groups, failed_groups = set(), set()
    dt_u32 = U32
    for b in range(B):
        p = pos[b]
        keys = torch.cat([K[b, :, :p].cpu().double(), kfresh[b][:, None]], 1)        # [heads, n, 128]
        vals = torch.cat([V[b, :, :p].cpu().double(), vfresh[b][:, None]], 1)
        qb = qrot[b]
        s = SCALE * (qb[:, None] @ keys.transpose(1, 2))                            # [heads, 1, n]
        out, absv, pr, den = softmax_pv(s, vals)                                    # [heads, 1, 128]
        out, absv, pr, den = out[:, 0], absv[:, 0], pr[:, 0], den[:, 0]
        sabs = SCALE * (keys.abs() @ qb.abs()[:, :, None]).squeeze(-1)
        dq = SCALE * (keys.abs() @ qamb[b][:, :, None]).squeeze(-1)
        dk = SCALE * (kamb[b] * qb.abs()).sum(-1)
        delta = 16 * dt_u32 * sabs.amax(-1) + dq.amax(-1) + dk
        gamma = (p + 1) / 8 * dt_u32 + 64 * dt_u32
        bd = ulp(out, dt) + (gamma + torch.expm1(2 * delta))[:, None] * absv
        ref[b], bound[b] = out, bd
        # negative controls
        if p >= 1:
            o, *_ = softmax_pv(s[..., :p], vals[:, :p])
            fails["fresh key dropped"] |= bool(bound_fails(o[:, 0], out, bd).any())
            keep = torch.ones(p + 1, dtype=torch.bool)
            keep[p - 1] = False
            o, *_ = softmax_pv(s[..., keep], vals[:, keep])
            fails["last cached key dropped"] |= bool(bound_fails(o[:, 0], out, bd).any())
        for d, key in ((1, "q rotated at pos + 1"), (-1, "q rotated at pos - 1")):
            qw, _ = rotate(q[b], torch.tensor(p + d), dt)
            o, *_ = softmax_pv(SCALE * (qw[:, None] @ keys.transpose(1, 2)), vals)
            fails[key] |= bool(bound_fails(o[:, 0], out, bd).any())
        if p >= 1:                               # one 16-key group of the cached keys removed, every group at once
            G = (p + 15) // 16
            pv = torch.zeros(heads, G * 16, HD, dtype=torch.float64)
            pw = torch.zeros(heads, G * 16, dtype=torch.float64)
            pv[:, :p] = pr[:, :p, None] * vals[:, :p]
            pw[:, :p] = pr[:, :p]
            num = (pr[:, :, None] * vals).sum(1)
            og = (num[:, None] - pv.view(heads, G, 16, HD).sum(2)) / (den[:, None] - pw.view(heads, G, 16).sum(2)[..., None])
            bad = bound_fails(og, out[:, None], bd[:, None]).any(-1).any(0)
            failed_groups |= set(bad.nonzero().flatten().tolist())
            spike_groups |= {int(t) // 16 for t in spike[b] if t < p}
    for key, failed in fails.items():
        assert failed, f"negative control '{key}' passes the bound in case {name}: bound or inputs too weak"
    assert spike_groups <= failed_groups, f"removing 16-key groups {sorted(spike_groups - failed_groups)[:8]} passes the bound in case {name}"
    if mode == "groups":
        assert len(failed_groups) == MAX_POS // 16
    return dict(pos=pos, max_seq=max_seq, qkv=qkv, K=K, V=V, rows=rows, kdom=kdom, vdom=vdom, kfresh=kfresh, kamb=kamb, vfresh=vfresh,
                ref=ref.reshape(B, H), bound=bound.reshape(B, H))


DECODE_GRID = [(name, dt, heads, split) for name in DECODE_CASES for dt in (torch.float16, torch.bfloat16) for heads in (32, 40)
               for split in (0, 1, 2, 4, 8)]


@pytest.mark.parametrize("name,dt,heads,split", DECODE_GRID,
                         ids=[f"{n}-{'f16' if d == torch.float16 else 'bf16'}-h{h}-split{s}" for n, d, h, s in DECODE_GRID])
def test_decode_attention_vs_fp64(ctx, models, name, dt, heads, split):
    """Ragged positions in one launch (0 .. 4095, +-1 around 16/32/64/128/256/1024 boundaries), a max_seq that is not a multiple of 64 filled
    to its last row, B = 1 / 8 / 17 / 20 / 64; every split.  Per launch: outputs within the bound; row pos of both caches = the rotated k
    (exact where the rounding is unambiguous, else within 1 ulp or the fp32 error) and v, every other byte of both caches unchanged; the arrival tickets back at zero; three
    launches bitwise equal; the NaN/Inf and the dominating poison past pos give the same bits; a sequence launched alone gives its row's bits."""
    from video_llava_amd import _lib
    cs = decode_case(name, dt, heads)
    llm = models[(dt, heads)]
    pos, max_seq = cs["pos"], cs["max_seq"]
    B, H = len(pos), heads * HD
    part = torch.full((B * heads * 8 * (HD + 2),), math.nan, dtype=torch.float32, device=DEV)
    ticket = torch.zeros(B * heads, dtype=torch.int32, device=DEV)
    K, V = cs["K"].clone(), cs["V"].clone()
    outs = []
    for _ in range(3):
        out = torch.full((B, H), math.nan, dtype=dt, device=DEV)
        _lib.check(decode_call(ctx, llm, cs["qkv"], pos, K, V, out, max_seq, split, part, ticket), "pgv_decode_attention")
        torch.cuda.synchronize()
        assert int(ticket.abs().sum()) == 0, "split merge left a ticket armed"
        outs.append(out)
    for o in outs[1:]:
        assert torch.equal(bits(o), bits(outs[0])), "repeated launches differ"

    # the cache append: row pos of every (b, h), nothing else
    bi = torch.arange(B, device=DEV)
    pd = torch.tensor(pos, device=DEV)
    krow, vrow = K[bi, :, pd].cpu().double(), V[bi, :, pd].cpu().double()          # [B, heads, 128]
    kf, kamb = cs["kfresh"], cs["kamb"]
    assert torch.equal(vrow, cs["vfresh"]), "v appended inexactly"
    assert_rotation(krow, kf, kamb, dt, "appended k")
    for new, old in ((K, cs["K"]), (V, cs["V"])):
        diff = bits(new) != bits(old)
        diff[bi, :, pd] = False
        assert not diff.any(), f"cache bytes outside row pos changed: first at {diff.nonzero()[0].tolist()}"

    # the dominating finite poison past pos (row pos too) must not change a bit
    Kd = torch.where(cs["rows"], cs["kdom"], cs["K"])
    Vd = torch.where(cs["rows"], cs["vdom"], cs["V"])
    outd = torch.full((B, H), math.nan, dtype=dt, device=DEV)
    _lib.check(decode_call(ctx, llm, cs["qkv"], pos, Kd, Vd, outd, max_seq, split, part, ticket), "pgv_decode_attention")
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0
    assert torch.equal(bits(outd), bits(outs[0])), "poison past pos changed the output"
    del Kd, Vd

    # a sequence alone (its own part / ticket) = its row of the wide launch
    for b in sorted({0, B - 1, int(np.argmax(pos))}):
        Kb, Vb = cs["K"][b:b + 1].clone(), cs["V"][b:b + 1].clone()
        ob = torch.full((1, H), math.nan, dtype=dt, device=DEV)
        tb = torch.zeros(heads, dtype=torch.int32, device=DEV)
        _lib.check(decode_call(ctx, llm, cs["qkv"][b:b + 1], [pos[b]], Kb, Vb, ob, max_seq, split, part, tb), "pgv_decode_attention")
        torch.cuda.synchronize()
        assert int(tb.abs().sum()) == 0
        assert torch.equal(bits(ob[0]), bits(outs[0][b])), f"sequence {b} alone differs from its row of the {B}-sequence launch"

    assert_within(outs[0].cpu().double(), cs["ref"], cs["bound"], f"decode {name}")


# --------------------------------------------------------------------------------------------------
# prefill
# --------------------------------------------------------------------------------------------------
PF_LENS = [1, 2, 31, 32, 33, 127, 128, 129, 255, 257, 600]
PF_KOFF = [0, 1, 63, 64, 65, 130, 0, 1, 64, 130, 65]
QK_STD = 5.0 ** 0.5                              # score std 5: sharply peaked rows


def prefill_inputs(lens, koff, heads, max_seq, dt, seed):
    B, H, M = len(lens), heads * HD, sum(lens)
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(M, 3 * H, generator=g, device=DEV)
    qkv[:, :2 * H] *= QK_STD
    K = (torch.randn(B, heads, max_seq, HD, generator=g, device=DEV) * QK_STD).to(dt)     # rows [0, koff): the cached prefix
    V = torch.randn(B, heads, max_seq, HD, generator=g, device=DEV).to(dt)
    Tk = torch.tensor([o + n for o, n in zip(koff, lens)], device=DEV)
    past = torch.arange(max_seq, device=DEV)[None, None, :, None] >= Tk[:, None, None, None]
    return qkv.to(dt), K, V, past


def prefill_run(ctx, llm, qkv, lens, koff, K, V, max_seq, dt, H):
    from video_llava_amd import _lib
    q2 = qkv.clone()
    out = torch.full((sum(lens), H), math.nan, dtype=dt, device=DEV)
    _lib.check(prefill_call(ctx, llm, q2, lens, koff, K, V, out, max_seq), "pgv_prefill_attention")
    torch.cuda.synchronize()
    return q2, out


def prefill_check(name, dt, heads, lens, koff, qkv0, qkv1, K0, K1, V0, V1, out, head_sample=None):
    """Rotation write-back, cache append, and the outputs against the float64 bound; negative controls."""
    B, H = len(lens), heads * HD
    cu = np.concatenate([[0], np.cumsum(lens)])
    heads_ref = list(range(heads)) if head_sample is None else head_sample
    assert torch.equal(bits(qkv1[:, H:]), bits(qkv0[:, H:])), "prefill changed k / v in the qkv buffer"
    fails = {k: False for k in ("fresh key dropped", "last cached key dropped", "masked row leaked", "q rotated at pos + 1", "q rotated at pos - 1")}
    touched = torch.zeros(K0.shape[:3], dtype=torch.bool, device=DEV)
    for b in range(B):
        n, off = lens[b], koff[b]
        Tk = off + n
        touched[b, :, off:Tk] = True
        qpos = torch.arange(off, Tk)
        rows = slice(int(cu[b]), int(cu[b + 1]))
        q_in = qkv0[rows, :H].view(n, heads, HD).cpu()
        q_out = qkv1[rows, :H].view(n, heads, HD).cpu().double()
        qr, qamb = rotate(q_in, qpos[:, None], dt)
        assert_rotation(q_out, qr, qamb, dt, f"{name}: rotated q of sequence {b}")
        kr, kamb = rotate(qkv0[rows, H:2 * H].view(n, heads, HD).cpu(), qpos[:, None], dt)
        k_out = K1[b, :, off:Tk].cpu().double().transpose(0, 1)                   # [n, heads, 128]
        assert_rotation(k_out, kr, kamb, dt, f"{name}: appended k of sequence {b}")
        assert torch.equal(bits(V1[b, :, off:Tk].transpose(0, 1)), bits(qkv0[rows, 2 * H:].view(n, heads, HD))), f"{name}: appended v inexact"
        # reference on the kernel's (checked) rotated q and cache rows
        keys = K1[b, heads_ref, :Tk].cpu().double()                                # [h, Tk, 128]
        vals = V1[b, heads_ref, :Tk].cpu().double()
        qh = q_out[:, heads_ref].transpose(0, 1)                                    # [h, n, 128]
        s = SCALE * qh @ keys.transpose(1, 2)                                       # [h, n, Tk]
        kidx, qp = torch.arange(Tk), qpos[:, None]
        causal = kidx[None, :] <= qp
        ref, absv, pr, den = softmax_pv(s, vals, causal)
        sabs = (SCALE * qh.abs() @ keys.abs().transpose(1, 2)).masked_fill(~causal, 0).amax(-1)   # [h, n]
        gamma = 2.0 ** -(MANT[dt] + 1) + (Tk / 8 + 64) * U32
        bd = ulp(ref, dt) + (gamma + torch.expm1(2 * 32 * U32 * sabs))[..., None] * absv
        if dt == torch.float16:
            bd = bd + 2.0 ** -25 * (causal.double() @ vals.abs()) / den
        got = out[rows].view(n, heads, HD)[:, heads_ref].transpose(0, 1).cpu().double()
        assert_within(got, ref, bd, f"prefill {name} sequence {b} (len {n}, koff {off})")
        # negative controls
        valid = qp >= 1
        for key, mask in (("fresh key dropped", kidx[None, :] < qp), ("last cached key dropped", causal & (kidx[None, :] != qp - 1)),
                          ("masked row leaked", kidx[None, :] <= qp + 1)):
            rowsel = valid[:, 0] if key != "masked row leaked" else (qpos + 1 < Tk)
            if not rowsel.any():
                continue
            o, *_ = softmax_pv(s[:, rowsel], vals, mask[rowsel])
            fails[key] |= bool(bound_fails(o, ref[:, rowsel], bd[:, rowsel]).any())
        for d, key in ((1, "q rotated at pos + 1"), (-1, "q rotated at pos - 1")):
            qw, _ = rotate(q_in, (qpos + d)[:, None], dt)
            o, *_ = softmax_pv(SCALE * qw[:, heads_ref].transpose(0, 1) @ keys.transpose(1, 2), vals, causal)
            fails[key] |= bool(bound_fails(o, ref, bd).any())
    for key, failed in fails.items():
        assert failed, f"negative control '{key}' passes the bound in prefill case {name}: bound or inputs too weak"
    for new, old in ((K1, K0), (V1, V0)):
        diff = (bits(new) != bits(old)).any(-1) & ~touched
        assert not diff.any(), f"{name}: cache rows outside [koff, koff + len) changed: first at {diff.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("heads", [32, 40])
def test_prefill_attention_vs_fp64(ctx, models, dt, heads):
    """Ragged lengths 1 .. 600 in one launch behind cached prefixes of 0, 1, 63, 64, 65 and 130 keys; max_seq 736 (not a multiple of 64).
    Outputs within the bound, q rotated in place and the appended k / v rows checked, nothing else in the caches touched; NaN/Inf or
    dominating poison past Tk = koff + len gives the same bits."""
    lens, koff, max_seq = PF_LENS, PF_KOFF, 736
    llm, H = models[(dt, heads)], heads * HD
    qkv0, K0, V0, past = prefill_inputs(lens, koff, heads, max_seq, dt, seed=7 + heads + MANT[dt])
    Kn = torch.where(past, nan_poison(K0.shape, dt), K0)
    Vn = torch.where(past, nan_poison(V0.shape, dt), V0)
    K1, V1 = Kn.clone(), Vn.clone()
    qkv1, out = prefill_run(ctx, llm, qkv0, lens, koff, K1, V1, max_seq, dt, H)
    Kd = torch.where(past, torch.full_like(K0, 100.0) * (1 - 2 * (torch.arange(HD, device=DEV) % 2)).to(dt), K0)
    Vd = torch.where(past, torch.full_like(V0, 1e4), V0)
    _, outd = prefill_run(ctx, llm, qkv0, lens, koff, Kd, Vd, max_seq, dt, H)
    assert torch.equal(bits(outd), bits(out)), "poison past Tk changed the output"
    del Kd, Vd
    prefill_check("ragged", dt, heads, lens, koff, qkv0, qkv1, Kn, K1, Vn, V1, out)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_prefill_attention_to_position_4095(ctx, models, dt):
    """596 rows behind a 3500-key prefix: the last query sits at position 4095 (the end of the RoPE table and of a 4096-row cache); the float64
    reference on a sample of heads, the rotation and append checks on all."""
    lens, koff, max_seq, heads = [596], [3500], 4096, 32
    llm, H = models[(dt, heads)], heads * HD
    qkv0, K0, V0, past = prefill_inputs(lens, koff, heads, max_seq, dt, seed=11 + MANT[dt])
    K1, V1 = K0.clone(), V0.clone()
    qkv1, out = prefill_run(ctx, llm, qkv0, lens, koff, K1, V1, max_seq, dt, H)
    prefill_check("to 4095", dt, heads, lens, koff, qkv0, qkv1, K0, K1, V0, V1, out, head_sample=[0, 13, 31])


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_prefill_append_is_bitwise_one_prefill(ctx, models, dt):
    """pgv.h: an appended row is bitwise the row of one full prefill.  Six prompts of 300 rows, each cut into two calls at 1, 63, 64, 65, 128 and
    299: the outputs and cache rows of both calls equal those of one call over the whole prompt."""
    S, cuts, heads, max_seq = 300, [1, 63, 64, 65, 128, 299], 32, 320
    B, H = len(cuts), heads * HD
    llm = models[(dt, heads)]
    qkv0, K0, V0, past = prefill_inputs([S] * B, [0] * B, heads, max_seq, dt, seed=23 + MANT[dt])
    K0 = torch.where(past, nan_poison(K0.shape, dt), K0)
    V0 = torch.where(past, nan_poison(V0.shape, dt), V0)
    Kf, Vf = K0.clone(), V0.clone()
    _, out_full = prefill_run(ctx, llm, qkv0, [S] * B, None, Kf, Vf, max_seq, dt, H)
    first = torch.cat([qkv0[b * S:b * S + c] for b, c in enumerate(cuts)])
    second = torch.cat([qkv0[b * S + c:(b + 1) * S] for b, c in enumerate(cuts)])
    Ks, Vs = K0.clone(), V0.clone()
    _, out1 = prefill_run(ctx, llm, first, cuts, None, Ks, Vs, max_seq, dt, H)
    _, out2 = prefill_run(ctx, llm, second, [S - c for c in cuts], cuts, Ks, Vs, max_seq, dt, H)
    got = torch.cat([torch.cat([out1[sum(cuts[:b]):sum(cuts[:b + 1])], out2[sum(S - c for c in cuts[:b]):sum(S - c for c in cuts[:b + 1])]])
                     for b in range(B)])
    assert torch.equal(bits(got), bits(out_full)), "a prompt cut into two calls differs from one call"
    assert torch.equal(bits(Ks), bits(Kf)) and torch.equal(bits(Vs), bits(Vf)), "cache rows of two calls differ from one call"


# --------------------------------------------------------------------------------------------------
# host-side argument checks (rejected before anything reaches the device)
# --------------------------------------------------------------------------------------------------
def test_attention_entries_reject_bad_arguments_on_the_host(ctx, models):
    from video_llava_amd import _lib
    dt, heads = torch.float16, 32
    llm, H = models[(dt, heads)], heads * HD
    buf = torch.zeros(4 * 3 * H, dtype=dt, device=DEV)
    part = torch.zeros(4 * heads * 8 * (HD + 2), dtype=torch.float32, device=DEV)
    ticket = torch.zeros(4 * heads, dtype=torch.int32, device=DEV)
    bad_decode = [([0], 16, 3), ([0], 16, 16), ([0], 16, -1), ([16], 16, 0), ([-1], 16, 0), ([0], 4097, 0), ([0], 0, 0)]
    for pos, max_seq, split in bad_decode:
        rc = decode_call(ctx, llm, buf, pos, buf, buf, buf, max_seq, split, part, ticket)
        assert rc == _lib.PGV_EINVAL, (pos, max_seq, split, rc)
    rc = ctx.lib.pgv_decode_attention(ctx.handle, llm, buf.data_ptr(), ints([0]), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0, 16, 0,
                                      part.data_ptr(), ticket.data_ptr(), _lib.stream_ptr())
    assert rc == _lib.PGV_EINVAL
    rc = ctx.lib.pgv_decode_attention(ctx.handle, llm, buf.data_ptr(), ints([0] * 65), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 65, 16, 0,
                                      part.data_ptr(), ticket.data_ptr(), _lib.stream_ptr())
    assert rc == _lib.PGV_EINVAL
    for lens, koff, max_seq in (([8], [9], 16), ([17], None, 16), ([0], None, 16), ([4], [-1], 16), ([1], None, 4097)):
        rc = prefill_call(ctx, llm, buf, lens, koff, buf, buf, buf, max_seq)
        assert rc == _lib.PGV_EINVAL, (lens, koff, max_seq, rc)
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0 and int(buf.float().abs().sum()) == 0, "a rejected call wrote to a buffer"
