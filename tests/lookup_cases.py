"""Shared checks of the row-wise decode step (tests/test_gpu_lookup.py and its child processes): `decode_rows` against consecutive `decode_step`
calls on the same tokens.  Everything is torch.equal; no tolerances."""
import numpy as np
import torch

DEV = "cuda:0"


def poison(m, vocab, W, max_seq, seed=991):
    """Fill all W slots of the (W, max_seq) cache with another group's rows (as tests/test_gpu_fork.py does)."""
    rng = np.random.default_rng(seed)
    n = min(max_seq, 90)
    kv, _, _ = m.prefill([[1] + rng.integers(3, vocab - 3, n - 1).tolist() for _ in range(W)], None, max_seq)
    return kv


def peek(m, kv, slot, row0, n):
    """K and V rows [row0, row0 + n) of every layer and head of `slot`, as bits."""
    L = m.config.num_hidden_layers
    return torch.stack([m.kv_peek(kv, l, w, slot, row0, n) for l in range(L) for w in (0, 1)]).view(torch.int16)


def check_rows_equal_steps(m, vocab, lens, rows, max_seq, seed):
    """Sequences of `lens` prompt tokens, rows[b] rows for sequence b: the logits of row j of sequence b and the cache rows the step wrote equal those
    of the j-th decode_step fed the same tokens."""
    rng = np.random.default_rng(seed)
    B, n = len(lens), max(rows)
    prompts = [[1] + rng.integers(3, vocab - 3, ln - 1).tolist() for ln in lens]
    toks = torch.from_numpy(rng.integers(3, vocab - 3, (B, n)).astype(np.int32)).to(DEV)
    poison(m, vocab, B, max_seq)
    kv, _, _ = m.prefill(prompts, None, max_seq)
    m.set_lookup(kv, n - 1)
    slots = [b for b in range(B) for _ in range(rows[b])]
    flat = torch.cat([toks[b, :rows[b]] for b in range(B)])
    got = m.decode_rows(kv, slots, flat)
    assert [m.kv_len(kv, b) for b in range(B)] == list(lens), "decode_rows must not advance the lengths"
    got_cache = [peek(m, kv, b, lens[b], rows[b]) for b in range(B)]
    assert torch.isfinite(got).all()
    first = np.cumsum([0] + list(rows[:-1])).tolist()
    for j in range(n):
        _, lg = m.decode_step(kv, toks[:, j].contiguous(), want_logits=True)
        for b in range(B):
            if j < rows[b]:
                assert torch.equal(got[first[b] + j], lg[b]), (lens, rows, b, j, float((got[first[b] + j] - lg[b]).abs().max()))
    for b in range(B):
        assert torch.equal(got_cache[b], peek(m, kv, b, lens[b], rows[b])), (lens, rows, b)
    m.set_lookup(kv, 0)
