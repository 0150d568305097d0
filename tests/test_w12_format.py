"""CPU: the lossless 12-bit weight stream (video_llava_amd/csrc/w12.h) in its numpy twin -- encode then decode is the identity on every bf16
bit pattern, and on the bench's own weights it costs at most 12.1 bits per weight with few exceptions."""
import numpy as np
import pytest
import torch

import w12_numpy as w12


def _roundtrip(bits):
    buf, counts = w12.encode(bits)
    assert counts.max() <= w12.MAX_EXC, counts.max()
    back = w12.decode(buf, *bits.shape)
    assert np.array_equal(back, bits)
    return buf, counts


@pytest.mark.parametrize("name", ["self_attn.q_proj.weight", "mlp.gate_proj.weight", "mlp.down_proj.weight"])
def test_bench_init_matrices_roundtrip_and_cost(name):
    from video_llava_amd import random_init as ri
    key = "model.layers.0." + name
    w = next(t for k, t in ri.iter_llama_tensors(vocab=64, layers=1, device="cpu", dtype=torch.bfloat16, seed=7) if k == key)
    bits = w12.bf16_bits(w)
    buf, counts = _roundtrip(bits)
    N, K = bits.shape
    bpw = buf.size * 8 / (N * K)
    rate = counts.sum() / (N * K)
    print(f"{name} {N}x{K}: {bpw:.4f} bits/weight, exceptions {100 * rate:.4f} % of weights, at most {counts.max()} per 16-row block")
    assert bpw <= 12.1 and rate < 5e-4


def test_adversarial_rows_roundtrip():
    rng = np.random.default_rng(3)
    N, K = 64, 256
    bits = w12.bf16_bits((torch.randn(N, K, generator=torch.Generator().manual_seed(5)) * 0.02).to(torch.bfloat16)).copy()
    bits[0] = 0                                                            # a row of zeros
    bits[1] = rng.choice(np.array([0x0000, 0x8000], np.uint16), K)         # +0 / -0
    bits[2] = rng.integers(1, 0x80, K).astype(np.uint16) | (rng.integers(0, 2, K).astype(np.uint16) << 15)   # subnormals of either sign
    bits[3, :8] = [0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81, 0x0000, 0x8000, 0x0001]                        # Inf, -Inf, NaNs, zeros, a subnormal
    bits[4, 17] = 0x7F7F                                                   # one huge outlier (largest finite)
    bits[5] = 0x3F80                                                       # all equal (1.0)
    bits[6, ::8] = rng.integers(0, 1 << 16, K // 8).astype(np.uint16)      # arbitrary bit patterns: many exceptions
    bits[7] = 0x7FC0                                                       # a row of NaNs
    bits[8] = 0xFF80                                                       # a row of -Inf
    bits[63, -1] = 0x0001                                                  # the last unit's last weight
    _roundtrip(bits)
    base = w12.row_bases(bits)
    assert base[0] == 0 and base[5] == 0x3F and base[4] == w12.row_bases(bits[4:5, :].copy())[0]
    # the outlier did not move the row base: it is the row's only exception
    _, counts = w12.encode(bits[:16])
    assert counts[0] > 0


def test_every_bit_pattern_roundtrips():
    """All 65536 bf16 patterns, two per row of 256 next to typical weights (at most 64 exceptions per 16-row block, the format's limit), so
    every pattern is coded against a base of real weights -- in the window or as an exception."""
    rng = np.random.default_rng(11)
    pats = rng.permutation(np.arange(1 << 16, dtype=np.uint32)).astype(np.uint16).reshape(-1, 2)
    rows = pats.shape[0]
    bits = w12.bf16_bits((torch.randn(rows, 256, generator=torch.Generator().manual_seed(2)) * 0.02).to(torch.bfloat16)).copy()
    cols = np.stack([rng.choice(256, 2, replace=False) for _ in range(rows)])
    bits[np.arange(rows)[:, None], cols] = pats
    _roundtrip(bits)
