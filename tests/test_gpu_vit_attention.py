"""CLIP attention (csrc/vit_attn.hip, through pgv_vit_attention of the C ABI) checked element by element against a float64 reference, on inputs
that are PROVEN to drive each of the kernel's data-dependent softmax routes.  The tests marked `gpu` launch the kernel; the others (route
predictions with their margins, negative controls) are host arithmetic and run anywhere.

Reference.  q, k, v as the dtype's values in float64, scores * 64^-0.5, exact softmax, PV, per (frame, head).

Routes.  A query block of 32 takes its first chunk of 96 keys exactly (chunk maximum, rescale from the empty state) and every later chunk by one of
  1  speculative: p = exp2(s - mrun) with the running maximum as it stands, accepted when every one of the 64 lane sums is <= 4096;
  2  speculation failed: scores recomputed, V reloaded, mask reapplied, then
  3  exact with rescale when some query's chunk maximum exceeds its mrun + 6: mnew = max(mrun, cmax) per query, alpha = exp2(mrun - mnew).
With finite inputs route 2 without route 3 cannot occur: a lane sums at most 48 scores, so a sum above 4096 needs one p > 85.3 = 2^6.4, that is a
score more than 6.4 units above mrun, which is more than the 6 the rescale asks for.  `kernel_model` below replays these decisions in float64 with
mrun tracked as the kernel tracks it (raised only by a rescale).  A lane (query q, half hi) holds the keys with ((key mod 32) div 4) mod 2 == hi:
mask() numbers a lane's 16 scores of a block key = 32 blk + 4 hi + (e & 3) + 8 (e >> 2).  Every case asserts the routes it claims with a margin
of >= 0.25 log2 units between log2(largest lane sum) and 12, and between max_q(cmax - mrun) and 6 wherever that second test is evaluated (only after
a failed speculation, where the argument above already puts it >= 0.4 beyond).  The kernel's own score error (Delta below) is five orders of
magnitude smaller, so a decisive prediction is the route the kernel takes.

Bound, per output element: |out - ref| <= ulp_dtype(ref) + (gamma + expm1(2 Delta)) * sum_i p_i |v_i| / sum_i p_i  (+ a subnormal term, fp16)
  ulp_dtype(ref)  the final rounding of the fp32 result to the dtype (half an ulp) with as much again for everything below.
  Delta           bound on the error of every score (natural-log units); |ds_i| <= Delta moves every softmax weight by a factor within
                  [e^-2Delta, e^2Delta].  In units of u32 * S_abs (u32 = 2^-24, S_abs = max over keys of 64^-0.5 sum_e |q_e k_e|):
                    64   the 64 exact 16-bit products summed in fp32 by 4 chained 32x32x16 MFMAs.  The order inside an MFMA is not documented;
                         one rounding per addition bounds every order
                     4   x = s * c - mrun: the rounded constant c = fp32(64^-0.5 log2 e) (1), the product (1, none if contracted to an FMA) and
                         the rounding of x, |x| <= |s| + |mrun| <= 2 S_abs (2).  The rounding of mrun = cmax * c itself is common to all keys
                         of a query and cancels
                  2 nch  alpha = exp2(mrun - mnew): the fp32 difference, <= 2 S_abs in magnitude, rounds once per rescale, at most nch = number
                         of chunks times, and acts on every key absorbed before it like a score error
  gamma           u_dtype  P is rounded to the dtype for the PV MFMA while the normaliser is summed from the unrounded fp32 values
                  + (npad + 3 nch + 48) u32:  npad for the fp32 PV sums (npad / 16 chained MFMAs of 16 products, one rounding per addition);
                  3 nch for o *= alpha, lrun *= alpha and lrun += psum; 48 for v_exp_f32 on numerator and denominator (2 + 2), alpha's own
                  exp2 (cancels: same value on both sides), the lane's 24 + 1 + 1 packed partial sums and the cross-half sum (27), 1 / ltot and
                  the final product (3), the rest slack for second-order terms.
  fp16 P < 2^-14  T::from_f32 is a plain conversion (v_cvt_f16_f32) and the library is built without denormal flushing, so a subnormal P is ROUNDED
                  to a multiple of 2^-24 (absolute error <= 2^-25, P < 2^-25 becomes 0), not flushed, and the MFMA reads subnormal inputs as they
                  are.  The kernel's mrun never exceeds the true running maximum, so its P is never smaller than the reference's p / max and only
                  keys with p / max < 2^-14 can be affected (2^-13 taken here); later rescales only shrink the error: + 2^-25 sum_{those} |v| / sum p.
                  bf16 has fp32's exponent range: nothing to add.

Inputs.  Background q / k with score std 0.18 (flat), v ~ 8 N(0,1); on top of it, per (frame, head) unit of one launch: one hot key 20 .. 40 log2
units above the rest for one query (v = +-48 .. 96 with alternating sign), placed at the first and last key of every later chunk and for a query of
the first, a middle and the last partial block; a ramp of +13 per chunk (every later chunk fails and rescales), a ramp of +9 (every other chunk
accepted with mrun 9 below the true maximum: the lazy state), a falling ramp (peak in chunk 0, later keys 40 below with ten keys spread over fp16's
subnormal range), flat units and ordinary peaked ones (score std 4), so routes differ between neighbouring workgroups.  Negative controls evaluate
the same bound against broken float64 models and require each to fail it.
"""
import functools
import math
import time

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"

HD = 64
SCALE = HD ** -0.5
LOG2E = 1.4426950408889634
S2 = SCALE * LOG2E                               # raw score -> log2 units
U32 = 2.0 ** -24
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}
DTYPES = [torch.float16, torch.bfloat16]
DTN = {torch.float16: "f16", torch.bfloat16: "bf16"}
SPEC_LOG2, LAZY_TH, MARGIN = 12.0, 6.0, 0.25
GUARD = 3                                        # rows behind T * N that must stay untouched

STATS = {"tests": 0, "t0": None, "worst": {}, "routes": {}}        # printed by every GPU test: the last line holds the suite's totals


def ulp(x, dt):
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** EMIN[dt]))
    return torch.ldexp(torch.ones_like(x), e - 1 - MANT[dt])


def bound_fails(out, ref, bound):
    return ~((out - ref).abs() <= bound)          # NaN fails


# --------------------------------------------------------------------------------------------------
# float64 model of the kernel's route decisions (and, for the negative controls, of its accumulation)
# --------------------------------------------------------------------------------------------------
def kernel_model(s2, v=None, defect=None):
    """s2 [U, N, N] scores in log2 units (float64), v [U, N, 64].  Returns dict(route [U, nkb, nch] with 0 = first chunk, 1 = speculation accepted,
    3 = speculation failed + rescale, 2 = failed without rescale; spec [U, nkb, nch] = log2 of the largest lane sum (nan in chunk 0);
    gap = max_q(cmax - mrun) where the rescale test is evaluated, else nan; lag = max_q(true running maximum - mrun) at the time the chunk is
    absorbed; out = o / l when v is given).  `defect` plants one wrong step into the accumulation:
      o_kept / l_kept / o_half   at a rescale behind chunk 0 the accumulator (all of it / its upper 32 columns) or the row sum is not scaled
      shared_max_f16             a rescaling block uses one maximum for its 32 queries, P rounded to fp16 in the numerator
      nomask_refail              the padded keys of the last block (copies of key N - 1) are counted after a failed speculation
      rem2_one_block             a last chunk of two blocks absorbs only the first"""
    U, N, _ = s2.shape
    nkb = (N + 31) // 32
    npad = nkb * 32
    s = s2[:, torch.arange(npad).clamp_max(N - 1)]                      # rows past N re-read the last query
    half = ((torch.arange(N) % 32) // 4) % 2
    starts = list(range(0, nkb, 3))
    nch = len(starts)
    route = torch.zeros(U, nkb, nch, dtype=torch.long)
    spec = torch.full((U, nkb, nch), math.nan, dtype=torch.float64)
    gap = torch.full_like(spec, math.nan)
    lag = torch.zeros_like(spec)
    mrun = torch.full((U, npad), -math.inf, dtype=torch.float64)
    mtrue = mrun.clone()
    lrun = torch.zeros(U, npad, dtype=torch.float64)
    o = torch.zeros(U, npad, HD, dtype=torch.float64) if v is not None else None
    for ci, kb0 in enumerate(starts):
        k0, k1 = kb0 * 32, min((kb0 + 3) * 32, N)
        if defect == "rem2_one_block" and nkb - kb0 == 2:
            k1 = k0 + 32
        sc, hm = s[:, :, k0:k1], half[k0:k1]
        cm = sc.amax(-1)
        if ci == 0:
            resc = torch.ones(U, nkb, dtype=torch.bool)
            fail = resc
        else:
            e = torch.exp2(sc - mrun[..., None])
            lane = torch.maximum((e * (hm == 0)).sum(-1), (e * (hm == 1)).sum(-1))
            spec[:, :, ci] = torch.log2(lane.view(U, nkb, 32).amax(-1))
            fail = spec[:, :, ci] > SPEC_LOG2
            g = (cm - mrun).view(U, nkb, 32).amax(-1)
            gap[:, :, ci] = torch.where(fail, g, torch.full_like(g, math.nan))
            resc = fail & (g > LAZY_TH)
            route[:, :, ci] = torch.where(resc, 3, torch.where(fail, 2, 1))
        rq = resc.repeat_interleave(32, 1)                                # per query
        mnew = torch.where(rq, torch.maximum(mrun, cm), mrun)
        if defect == "shared_max_f16" and ci > 0:
            mnew = torch.where(rq, mnew.view(U, nkb, 32).amax(-1, keepdim=True).expand(U, nkb, 32).reshape(U, npad), mnew)
        alpha = torch.exp2(mrun - mnew)                                   # exp2(-inf) = 0 on the first chunk
        mrun = mnew
        mtrue = torch.maximum(mtrue, cm)
        lag[:, :, ci] = (mtrue - mrun).view(U, nkb, 32).amax(-1)
        p = torch.exp2(sc - mrun[..., None])
        psum = p.sum(-1)
        later = rq & (ci > 0)
        if v is not None:
            pn = p
            if defect == "shared_max_f16":
                pn = torch.where(later[..., None], p.half().double(), p)
            ao = alpha
            if defect == "o_kept":
                ao = torch.where(later, torch.ones_like(alpha), alpha)
            o = o * ao[..., None]
            if defect == "o_half":
                o[..., 32:] = torch.where(later[..., None], o[..., 32:] / alpha.clamp_min(1e-300)[..., None], o[..., 32:])
            o = o + pn @ v[:, k0:k1]
        lrun = lrun * (torch.where(later, torch.ones_like(alpha), alpha) if defect == "l_kept" else alpha) + psum
        if defect == "nomask_refail" and ci > 0 and k1 == N and npad > N:
            extra = (npad - N) * p[..., -1] * fail.repeat_interleave(32, 1)
            lrun = lrun + extra
            if v is not None:
                o = o + extra[..., None] * v[:, N - 1][:, None]
    res = dict(route=route, spec=spec, gap=gap, lag=lag, nch=nch, nkb=nkb)
    if v is not None:
        res["out"] = (o / lrun[..., None])[:, :N]
    return res


def margins(m):
    """Smallest distance of any evaluated decision from its threshold, log2 units."""
    a = (m["spec"] - SPEC_LOG2).abs()
    b = (m["gap"] - LAZY_TH).abs()
    return float(torch.nan_to_num(torch.minimum(torch.nan_to_num(a, nan=math.inf), torch.nan_to_num(b, nan=math.inf)), posinf=1e9).min())


def reference(q, k, v, dt):
    """q, k, v [U, N, 64] float64 (dtype values).  Returns ref, bound [U, N, 64], the max-normalised weights p [U, N, N] and s2."""
    U, N, _ = q.shape
    npad = (N + 31) // 32 * 32
    nch = (npad // 32 + 2) // 3
    sraw = q @ k.transpose(1, 2)
    s = SCALE * sraw
    p = torch.exp(s - s.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    ref = p @ v / den
    absv = p @ v.abs() / den
    sabs = (SCALE * q.abs() @ k.abs().transpose(1, 2)).amax(-1)
    delta = (68 + 2 * nch) * U32 * sabs
    gamma = 2.0 ** -(MANT[dt] + 1) + (npad + 3 * nch + 48) * U32
    bound = ulp(ref, dt) + (gamma + torch.expm1(2 * delta))[..., None] * absv
    if dt == torch.float16:
        bound = bound + 2.0 ** -25 * ((p < 2.0 ** -13).double() @ v.abs()) / den
    return ref, bound, p, S2 * sraw


def split_qkv(qkv):
    """qkv [T, N, 3, heads, 64] (dtype) -> q, k, v [T * heads, N, 64] float64."""
    T, N, _, H, _ = qkv.shape
    x = qkv.double().permute(2, 0, 3, 1, 4).reshape(3, T * H, N, HD)
    return x[0], x[1], x[2]


# --------------------------------------------------------------------------------------------------
# constructed units
# --------------------------------------------------------------------------------------------------
HOT_DIM, RAMP_DIM = 40, 48


def background(N, g, peaked=False):
    """Flat: q / k on 32 columns, score std 0.18.  Peaked: score std 4 (the ordinary sharply peaked head)."""
    q, k = torch.zeros(N, HD), torch.zeros(N, HD)
    if peaked:
        q, k = torch.randn(N, HD, generator=g) * 2.0, torch.randn(N, HD, generator=g) * 2.0
    else:
        q[:, :32], k[:, :32] = torch.randn(N, 32, generator=g) * 0.5, torch.randn(N, 32, generator=g) * 0.5
    return q, k, torch.randn(N, HD, generator=g) * 8.0


def big_v(scale=48.0):
    d = torch.arange(HD)
    return scale * (1 - 2 * (d % 2)).float() * (1 + d / 64.0)


def chunk_of(key):
    return key // 96


def make_unit(kind, N, g, dt, **a):
    """One (frame, head): (q, k, v [N, 64] fp32 values, claim).  claim: dict(kind, and what the predictor must report)."""
    nkb = (N + 31) // 32
    nch = (nkb + 2) // 3
    q, k, v = background(N, g, peaked=(kind == "peaked"))
    claim = dict(kind=kind)
    if kind == "hot":
        kpos, qpos, L = a["kpos"], a["qpos"], a["L"]
        amp = math.sqrt(L / S2)
        k[kpos, HOT_DIM] = amp
        q[qpos, HOT_DIM] = amp
        v[kpos] = big_v() * (-1.0 if a.get("neg") else 1.0)
        claim.update(kpos=kpos, qpos=qpos, L=L, block=qpos // 32, chunk=chunk_of(kpos))
    elif kind in ("ramp13", "ramp9"):
        step = 18.0 if kind == "ramp13" else 12.5                      # * 4 * S2 = 12.98 / 9.02 log2 units; exact in fp16 and bf16
        q[:, RAMP_DIM] = 4.0
        for c in range(nch):
            lo, hi = 96 * c, min(96 * c + 96, N)
            pc = lo + (37 * c + 5) % (hi - lo)
            k[pc] = 0
            k[pc, RAMP_DIM] = step * (c + 1)
            v[pc] = big_v() * (1.0 if c % 2 else -1.0)
    elif kind == "falling":
        q[:, RAMP_DIM] = 4.0
        k[7] = 0
        k[7, RAMP_DIM] = 55.5                                           # 40.04 log2 units above the background
        v[7] = big_v()
        v[7, 32:] = 0
        for i, gdepth in enumerate(range(15, 25)):                      # p / max = 2^-15 .. 2^-24: fp16's subnormal range
            pos = 96 + (53 * i) % (N - 96)
            k[pos] = 0
            k[pos, RAMP_DIM] = round((40.04 - gdepth) / (4 * S2) * 8) / 8
            v[pos] = big_v(200.0) * (-1.0 if i % 2 else 1.0)
    return q.to(dt), k.to(dt), v.to(dt), claim


def hot_placements(N):
    nkb = (N + 31) // 32
    nch = (nkb + 2) // 3
    keys = []
    for c in range(1, nch):
        for kp in (96 * c, min(96 * c + 95, N - 1)):
            if kp not in keys:
                keys.append(kp)
    if N - 1 not in keys:
        keys.append(N - 1)
    queries = [5, 32 * (nkb // 2) + 17, N - 1]
    return [(kp, qp) for kp in keys for qp in queries]


HOT_N = [257, 289, 321, 384, 577, 608]
HEADS = 16


@functools.lru_cache(maxsize=2)
def constructed_case(N, dt):
    """All constructed units of one token count in one launch of 16 heads: qkv [T, N, 3, 16, 64] and the per-unit claims."""
    g = torch.Generator().manual_seed(7919 * N + MANT[dt])
    specs = [("hot", dict(kpos=kp, qpos=qp, L=20.0 + (7 * i) % 21, neg=bool(i % 2))) for i, (kp, qp) in enumerate(hot_placements(N))]
    specs += [("ramp13", {}), ("ramp9", {}), ("falling", {}), ("flat", {}), ("peaked", {}), ("flat", {})]
    i = 0
    while len(specs) % HEADS:                                            # fill the last frame: flat and peaked heads side by side
        specs.append(("peaked" if i % 2 else "flat", {}))
        i += 1
    units = []
    for kind, a in specs:
        u = make_unit(kind, N, g, dt, **a)
        while kind == "peaked":                                          # an ordinary peaked head makes no claim but must be decisive too
            mq, mk = u[0].double()[None], u[1].double()[None]
            if margins(kernel_model(S2 * mq @ mk.transpose(1, 2))) >= MARGIN:
                break
            u = make_unit(kind, N, g, dt, **a)
        units.append(u)
    T = len(units) // HEADS
    qkv = torch.stack([torch.stack([u[j] for u in units]) for j in range(3)])          # [3, U, N, 64]
    qkv = qkv.view(3, T, HEADS, N, HD).permute(1, 3, 0, 2, 4).contiguous()
    return qkv, [u[3] for u in units]


def check_claims(N, dt, claims, model):
    """The routes every constructed unit claims, with margins; returns the route histogram over later (block, chunk) pairs."""
    route, nch, nkb = model["route"], model["nch"], model["nkb"]
    assert not (route == 2).any(), "speculation failed without a rescale: impossible with finite inputs"
    mg = margins(model)
    assert mg >= MARGIN, f"N={N} {DTN[dt]}: a route decision is only {mg:.3f} log2 units from its threshold: fix the input"
    later = route[:, :, 1:]
    for u, cl in enumerate(claims):
        r = later[u]
        if cl["kind"] == "hot":
            want = torch.ones_like(r)
            if cl["chunk"] >= 1:
                want[cl["block"], cl["chunk"] - 1] = 3
            assert torch.equal(r, want), f"unit {u} {cl}: routes {r.tolist()}"
        elif cl["kind"] == "ramp13":
            assert (r == 3).all(), f"unit {u} ramp13: routes {r.tolist()}"
        elif cl["kind"] == "ramp9":
            want = torch.tensor([1 if c % 2 else 3 for c in range(1, nch)]).expand(nkb, nch - 1)
            assert torch.equal(r, want), f"unit {u} ramp9: routes {r.tolist()}"
            acc = model["lag"][u][:, 1::2]
            assert (acc > 8.0).all(), f"unit {u} ramp9: accepted chunks must leave mrun several units below the true maximum, lag {acc.min():.2f}"
        elif cl["kind"] in ("falling", "flat"):
            assert (r == 1).all(), f"unit {u} {cl['kind']}: routes {r.tolist()}"
    return {k: int((later == k).sum()) for k in (1, 2, 3)}


@functools.lru_cache(maxsize=2)
def constructed_reference(N, dt):
    qkv, claims = constructed_case(N, dt)
    q, k, v = split_qkv(qkv)
    ref, bound, p, s2 = reference(q, k, v, dt)
    model = kernel_model(s2, v)
    assert ((model["out"] - ref).abs() <= 1e-9 * (1 + ref.abs())).all(), "the float64 chunked model disagrees with the plain softmax"
    hist = check_claims(N, dt, claims, model)
    return q, k, v, ref, bound, p, s2, hist


def softmax_pv(s2, v, keep=None, dup_last=False):
    if keep is not None:
        s2 = s2.masked_fill(~keep, -math.inf)
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    num, den = p @ v, p.sum(-1, keepdim=True)
    if dup_last:
        num, den = num + p[..., -1:] * v[:, -1:], den + p[..., -1:]
    return num / den


@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("N", HOT_N)
def test_constructed_routes_and_negative_controls(N, dt):
    """Host only.  Every constructed unit takes the routes it claims with >= 0.25 log2 units to both thresholds, and every broken float64 model
    leaves the bound on the units built for it."""
    q, k, v, ref, bound, p, s2, hist = constructed_reference(N, dt)
    _, claims = constructed_case(N, dt)
    nkb = (N + 31) // 32
    assert hist[3] > 0 and hist[1] > 0
    hot = [(u, c) for u, c in enumerate(claims) if c["kind"] == "hot" and c["chunk"] >= 1]
    models = {d: kernel_model(s2, v, d)["out"] for d in ("o_kept", "l_kept", "o_half", "nomask_refail", "rem2_one_block")}
    if dt == torch.float16:
        models["shared_max_f16"] = kernel_model(s2, v, "shared_max_f16")["out"]
    for u, c in hot:
        kp, qp, b = c["kpos"], c["qpos"], c["block"]
        keep = torch.ones(N, dtype=torch.bool)
        keep[kp] = False
        o = softmax_pv(s2[u:u + 1], v[u:u + 1], keep)
        assert bound_fails(o[0, qp], ref[u, qp], bound[u, qp]).any(), f"unit {u}: hot key dropped passes the bound"
        rows = slice(32 * b, min(32 * b + 32, N))
        for d in ("o_kept", "l_kept"):
            assert bound_fails(models[d][u, qp], ref[u, qp], bound[u, qp]).any(), f"unit {u}: {d} passes the bound on the hot row"
        assert not bound_fails(models["o_half"][u, rows, :32], ref[u, rows, :32], bound[u, rows, :32]).any()
        assert bound_fails(models["o_half"][u, qp, 32:], ref[u, qp, 32:], bound[u, qp, 32:]).any(), f"unit {u}: o_half passes the bound"
        if dt == torch.float16:
            riding = [r for r in range(rows.start, rows.stop) if r != qp]
            if riding:
                bad = bound_fails(models["shared_max_f16"][u, riding], ref[u, riding], bound[u, riding]).any(-1)
                # P = 2^-L: below 2^-25 it rounds to 0 and the chunk is lost; above, fp16's subnormal grid may still carry it inside the bound
                assert bad.any() and (c["L"] < 27 or bad.double().mean() > 0.75), f"unit {u}: riding queries computed with the hot query's maximum pass the bound"
        if kp == N - 1:
            o = softmax_pv(s2[u:u + 1], v[u:u + 1], dup_last=True)
            assert bound_fails(o[0], ref[u], bound[u]).any(), f"unit {u}: last valid key counted twice passes the bound"
        if chunk_of(kp) == chunk_of(N - 1) and N % 32 and rows.stop - rows.start > 1:      # the riding rows show it: the hot row's weight sits on the hot key either way
            assert bound_fails(models["nomask_refail"][u, rows], ref[u, rows], bound[u, rows]).any(), f"unit {u}: unmasked padding passes the bound"
    if nkb % 3 == 2:
        flat = [i for i, c in enumerate(claims) if c["kind"] in ("flat", "peaked")]
        assert bound_fails(models["rem2_one_block"][flat], ref[flat], bound[flat]).any(-1).any(-1).all(), "a two-block last chunk cut to one block passes the bound"
    for u in [i for i, c in enumerate(claims) if c["kind"] in ("flat", "peaked")][:2]:
        for b in range(nkb):                                             # one 32-key block removed, every block in turn
            keep = torch.ones(N, dtype=torch.bool)
            keep[32 * b:32 * b + 32] = False
            if keep.any():
                o = softmax_pv(s2[u:u + 1], v[u:u + 1], keep)
                assert bound_fails(o[0], ref[u], bound[u]).any(), f"unit {u}: key block {b} removed passes the bound"


# --------------------------------------------------------------------------------------------------
# launches
# --------------------------------------------------------------------------------------------------
def bits(x):
    return x.view(torch.int16)


def launch(ctx, dt, qkv_dev, T, N, heads, C_=None, expect_ok=True):
    """One call on a NaN-filled output with guard rows; returns (rc, out [T*N + GUARD, C])."""
    from video_llava_amd import _lib
    Cc = heads * HD if C_ is None else C_
    out = torch.full((T * N + GUARD, Cc), math.nan, dtype=dt, device=DEV)
    rc = ctx.lib.pgv_vit_attention(ctx.handle, _lib.dtype_code(dt), qkv_dev.data_ptr(), out.data_ptr(), T, N, Cc, heads, _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_ok:
        _lib.check(rc, "pgv_vit_attention")
    return rc, out


def run_and_check(ctx, dt, qkv, what, precomputed=None, unit_batch=32):
    """qkv [T, N, 3, heads, 64] (dtype, host).  The properties of every launch, then every element against the float64 bound."""
    if STATS["t0"] is None:
        STATS["t0"] = time.time()
    T, N, _, heads, _ = qkv.shape
    Cc = heads * HD
    dev = qkv.to(DEV)
    flat = dev.reshape(T * N, 3 * Cc)
    _, out = launch(ctx, dt, flat, T, N, heads)
    assert torch.isnan(out[T * N:].float()).all(), f"{what}: guard rows behind T * N were written"
    assert torch.isfinite(out[:T * N].float()).all(), f"{what}: non-finite or unwritten output"
    _, out2 = launch(ctx, dt, flat, T, N, heads)
    assert torch.equal(bits(out2), bits(out)), f"{what}: a second launch gives different bits"
    for t in sorted({0, T - 1}):                                          # frame t alone
        _, o1 = launch(ctx, dt, dev[t].reshape(N, 3 * Cc).contiguous(), 1, N, heads)
        assert torch.equal(bits(o1[:N]), bits(out[t * N:(t + 1) * N])), f"{what}: frame {t} alone differs from its rows of the {T}-frame launch"
    if heads > 1:                                                         # permuted head order
        perm = torch.randperm(heads, generator=torch.Generator().manual_seed(heads + N)).to(DEV)
        _, op = launch(ctx, dt, dev[:, :, :, perm].reshape(T * N, 3 * Cc).contiguous(), T, N, heads)
        want = out[:T * N].view(T * N, heads, HD)[:, perm].reshape(T * N, Cc)
        assert torch.equal(bits(op[:T * N]), bits(want)), f"{what}: permuted heads give different bits"
    got = out[:T * N].cpu().double().view(T, N, heads, HD).permute(0, 2, 1, 3).reshape(T * heads, N, HD)
    worst, U = 0.0, T * heads
    if precomputed is not None:
        ref, bound, hist = precomputed
        batches = [(slice(0, U), ref, bound)]
    else:                                                                 # reference and route model in batches of units: [U, N, N] float64 is large
        q, k, v = split_qkv(qkv)
        batches, hist = [], {1: 0, 2: 0, 3: 0}
        for u0 in range(0, U, unit_batch):
            sl = slice(u0, min(u0 + unit_batch, U))
            ref, bound, _, s2 = reference(q[sl], k[sl], v[sl], dt)
            m = kernel_model(s2)
            mg = margins(m)
            assert mg >= MARGIN, f"{what}: a route decision is only {mg:.3f} log2 units from its threshold: fix the input"
            for r in (1, 2, 3):
                hist[r] += int((m["route"][:, :, 1:] == r).sum())
            batches.append((sl, ref, bound))
    first_bad = None
    for sl, ref, bound in batches:
        g = got[sl]
        bad = bound_fails(g, ref, bound)
        worst = max(worst, float(((g - ref).abs() / bound).max()))
        if bad.any() and first_bad is None:
            idx = tuple(bad.nonzero()[0].tolist())
            first_bad = (f"{what}: {int(bad.sum())} elements outside the bound; first at unit {sl.start + idx[0]} query {idx[1]} column {idx[2]}: "
                         f"out {float(g[idx])!r} ref {float(ref[idx])!r} bound {float(bound[idx]):.3e}")
    STATS["tests"] += 1
    STATS["worst"][DTN[dt]] = max(STATS["worst"].get(DTN[dt], 0.0), worst)
    for r in (1, 2, 3):
        STATS["routes"][r] = STATS["routes"].get(r, 0) + hist[r]
    print(f"\n[vit-attn] {what}: worst error/bound {worst:.3f}; later (block, chunk) pairs by route {hist}; suite so far: {STATS['tests']} launches checked, "
          f"{time.time() - STATS['t0']:.1f} s, worst ratio {STATS['worst']}, routes {STATS['routes']}")
    assert first_bad is None, first_bad
    return out


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("N", HOT_N)
def test_vit_attention_constructed_routes_vs_fp64(ctx, N, dt):
    """One launch of 16 heads per token count whose (frame, head) units take, provably, every route of the online softmax: hot keys in every later
    chunk (first / last key, last chunks of 1, 2 and 3 blocks, the single valid key of a padded block), hot queries in the first, a middle and the
    last partial block, rising ramps (+13: every chunk fails and rescales; +9: lazy state), a falling ramp into fp16's subnormal range, flat and
    peaked heads side by side.  Routes and margins are asserted first, then every output element against the float64 bound."""
    qkv, _ = constructed_case(N, dt)
    q, k, v, ref, bound, p, s2, hist = constructed_reference(N, dt)
    run_and_check(ctx, dt, qkv, f"constructed N={N} {DTN[dt]}", precomputed=(ref, bound, hist))


# --------------------------------------------------------------------------------------------------
# shape edges with ordinary peaked inputs
# --------------------------------------------------------------------------------------------------
SHAPE_N = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 192, 193, 257, 288, 289, 320, 321, 352, 384, 385, 576, 577, 607, 608]
SHAPES = [(T, N, h) for N in SHAPE_N for T, h in ((3, 1), (2, 2), (1, 16))]
BIG = [(40, 257, 16), (20, 577, 16)]                 # 640 workgroups where two share a CU, 320 where one owns it: more than 256 CUs hold at once


def peaked_qkv(T, N, heads, dt, seed):
    """Score std 4 (3 .. 5 asked); a unit whose route decisions are not decisive is drawn again (fixing the input, never skipping the case)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.empty(T, N, 3, heads, HD, dtype=dt)
    for t in range(T):
        todo = list(range(heads))
        while todo:
            x = torch.randn(N, 3, len(todo), HD, generator=g)
            x[:, :2] *= 2.0
            x[:, 2] *= 3.0
            x = x.to(dt)
            qq, kk = x[:, 0].double().transpose(0, 1), x[:, 1].double().transpose(0, 1)
            m = kernel_model(S2 * qq @ kk.transpose(1, 2))
            a = torch.nan_to_num((m["spec"] - SPEC_LOG2).abs(), nan=math.inf).flatten(1).amin(1)
            b = torch.nan_to_num((m["gap"] - LAZY_TH).abs(), nan=math.inf).flatten(1).amin(1)
            ok = torch.minimum(a, b) >= MARGIN
            for j, h in enumerate(list(todo)):
                if ok[j]:
                    qkv[t, :, :, h] = x[:, :, j]
                    todo.remove(h)
    return qkv


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
@pytest.mark.parametrize("T,N,heads", SHAPES + BIG, ids=[f"T{T}-N{N}-h{h}" for T, N, h in SHAPES + BIG])
def test_vit_attention_shapes_vs_fp64(ctx, T, N, heads, dt):
    """Token counts around every boundary: one key, partial / exact / one-past 32-key blocks and 96-key chunks, N <= 96 (a single chunk, and with
    nkb < 4 waves that get no query block), 288 / 289 (the switch to 8 waves and two-part staging), last chunks of one, two and three blocks in the
    8-wave form (289, 321 / 352, 384), 576 / 577 and 607 / 608 (the LDS limit); 1, 2 and 16 heads; launches larger than the device holds at once."""
    qkv = peaked_qkv(T, N, heads, dt, seed=100003 * N + 17 * T + heads + MANT[dt])
    run_and_check(ctx, dt, qkv, f"peaked T={T} N={N} heads={heads} {DTN[dt]}")


def test_peaked_inputs_are_decisive():
    """Host only: the input builder of the shape cases leaves no route decision within 0.25 log2 units of a threshold (sample of the grid)."""
    for T, N, heads in [(2, 97, 2), (1, 257, 16), (1, 577, 16), (3, 608, 1)]:
        for dt in DTYPES:
            qkv = peaked_qkv(T, N, heads, dt, seed=100003 * N + 17 * T + heads + MANT[dt])
            q, k, _ = split_qkv(qkv)
            assert margins(kernel_model(S2 * q @ k.transpose(1, 2))) >= MARGIN


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.values())
def test_vit_attention_refuses_what_it_cannot_run(ctx, dt):
    """609 tokens need more than 160 KiB of LDS; a hidden size other than 64 * heads has no kernel.  Both are errors, and nothing is written."""
    from video_llava_amd import _lib
    for T, N, Cc, heads in ((1, 609, 128, 2), (2, 700, 64, 1), (1, 33, 96, 2), (1, 33, 128, 1), (1, 33, 1024, 8)):
        qkv = torch.randn(T * N, 3 * Cc, generator=torch.Generator().manual_seed(N)).to(dt).to(DEV)
        rc, out = launch(ctx, dt, qkv, T, N, heads, C_=Cc, expect_ok=False)
        assert rc != _lib.PGV_OK, f"T={T} N={N} C={Cc} heads={heads} was accepted"
        assert torch.isnan(out.float()).all(), f"T={T} N={N} C={Cc} heads={heads}: a refused call wrote to the output"
