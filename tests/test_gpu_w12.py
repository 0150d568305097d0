"""GPU: the lossless 12-bit weight stream of bf16 models (video_llava_amd/csrc/w12.h).  The device encoder writes byte for byte what its numpy
twin writes; the 12-bit GEMV equals the 16-bit GEMV bit for bit in every launch shape of one column tile; a model decodes the same tokens and
the same logits with the stream on and off, also after weights are reloaded."""
import numpy as np
import pytest
import torch

import w12_numpy as w12

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _encode(ctx, wb, N, K):
    from video_llava_amd import _lib
    nb = int(ctx.lib.pgv_w12_bytes(N, K))
    assert nb == w12.nbytes(N, K)
    buf = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(N // 16, dtype=torch.int32, device=DEV)
    _lib.check(ctx.lib.pgv_encode_w12_blocked(ctx.handle, _lib.dtype_code(torch.bfloat16), wb.data_ptr(), buf.data_ptr(), counts.data_ptr(), N, K,
                                              _lib.stream_ptr()))
    torch.cuda.synchronize()
    return buf, counts


def _blocked(ctx, w):
    from video_llava_amd import _lib
    N, K = w.shape
    wb = torch.zeros((N + 15) // 16 * 16, K, dtype=torch.bfloat16, device=DEV)
    _lib.check(ctx.lib.pgv_pack_blocked(ctx.handle, _lib.dtype_code(torch.bfloat16), w.to(DEV).contiguous().data_ptr(), N, K, wb.data_ptr(),
                                        _lib.stream_ptr()))
    return wb


def _adversarial(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    bits = w12.bf16_bits((torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)).copy()
    rng = np.random.default_rng(seed)
    bits[0] = 0
    bits[1] = rng.choice(np.array([0x0000, 0x8000], np.uint16), K)
    bits[2] = rng.integers(1, 0x80, K).astype(np.uint16) | (rng.integers(0, 2, K).astype(np.uint16) << 15)
    bits[3, :6] = [0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x0001, 0x8000]
    bits[4, K // 2 + 3] = 0x7F7F
    bits[5] = 0x3F80
    bits[6, rng.choice(K, 24, replace=False)] = rng.integers(0, 1 << 16, 24).astype(np.uint16)     # arbitrary bit patterns
    bits[7] = 0x7FC0
    bits[-1, -1] = 0x0001
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)


@pytest.mark.parametrize("N,K,kind", [(512, 4096, "bench"), (256, 11008, "bench"), (64, 512, "adversarial"), (48, 13824, "adversarial")])
def test_device_encoder_matches_numpy_twin(ctx, N, K, kind):
    if kind == "bench":
        w = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.02).to(torch.bfloat16)
    else:
        w = _adversarial(N, K, N + K)
    buf, counts = _encode(ctx, _blocked(ctx, w), N, K)
    ref, rcounts = w12.encode(w12.bf16_bits(w))
    assert np.array_equal(counts.cpu().numpy(), rcounts)
    assert rcounts.max() <= w12.MAX_EXC
    assert np.array_equal(buf.cpu().numpy(), ref)
    assert np.array_equal(w12.decode(ref, N, K), w12.bf16_bits(w))


def test_device_encoder_counts_overflowing_blocks(ctx):
    N, K = 32, 256
    bits = np.random.default_rng(1).integers(0, 1 << 16, (N, K)).astype(np.uint16)
    w = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    _, counts = _encode(ctx, _blocked(ctx, w), N, K)
    assert np.array_equal(counts.cpu().numpy(), w12.encode(bits)[1]) and int(counts.max()) > w12.MAX_EXC


# (mode, N, K): the shapes choose_gemv gives one column tile at 7B / 13B -- qkv three / four row blocks per workgroup, gate/up one (gate, up) pair,
# the producers and lm_head one row block (eight beyond 8 sequences) -- and short matrices where waves hold no group or a ragged last batch
SHAPES = [(0, 12288, 4096), (0, 15360, 5120), (2, 22016, 4096), (2, 27648, 5120), (1, 4096, 11008), (1, 5120, 13824), (3, 32003, 4096),
          (3, 32005, 5120), (0, 1536, 4096), (1, 512, 13824), (2, 1024, 192), (3, 515, 11008)]


@pytest.mark.parametrize("B", [1, 3, 8, 11, 16])
@pytest.mark.parametrize("mode,N,K", SHAPES)
def test_gemv_w12_bitwise_equals_16bit(ctx, mode, N, K, B):
    from video_llava_amd import _lib
    g = torch.Generator().manual_seed(N + K + B)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    bits = w12.bf16_bits(w).copy()
    # exceptions in the first unit, the last unit and the unit of the last (ragged) group of the middle row block
    bits[0, 0] = 0x0001; bits[0, 63] = 0x2F00; bits[N - 1, K - 1] = 0x8001; bits[N // 2, K - 64] = 0x4480; bits[N // 2 + 1, K - 33] = 0x0000
    w = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    x = torch.randn(B, K, generator=g).to(torch.bfloat16).to(DEV)
    dc = _lib.dtype_code(torch.bfloat16)
    wb = _blocked(ctx, w)
    Np = wb.shape[0]
    buf, counts = _encode(ctx, wb, Np, K)
    assert int(counts.max()) <= w12.MAX_EXC and int(counts[0]) >= 2 and int(counts[-1]) >= 1

    def out_buf():
        if mode == 0:
            return torch.empty(B, N, dtype=torch.bfloat16, device=DEV)
        if mode == 1:
            return torch.randn(B, N, generator=g).to(DEV)
        if mode == 2:
            return torch.empty(B, N // 2, dtype=torch.bfloat16, device=DEV)
        return torch.empty(B, N, dtype=torch.float32, device=DEV)
    o16 = out_buf()
    o12 = o16.clone()
    _lib.check(ctx.lib.pgv_gemv(ctx.handle, dc, mode, wb.data_ptr(), x.data_ptr(), K, o16.data_ptr(), o16.shape[1], N, K, B, _lib.stream_ptr()))
    _lib.check(ctx.lib.pgv_gemv_w12(ctx.handle, dc, mode, buf.data_ptr(), x.data_ptr(), K, o12.data_ptr(), o12.shape[1], N, K, B, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(o16, o12)


def _model(hidden, inter, heads, layers, vocab, seed):
    from video_llava_amd import random_init as ri
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    cfg = VideoChatGPTConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                             eos_token_id=None)
    m = VideoChatGPTLlamaForCausalLM(cfg, VisionConfig(frame_size=224), torch.bfloat16, torch.device(DEV))
    ri.load_streaming(m, ri.iter_llama_tensors(vocab=vocab, hidden=hidden, inter=inter, layers=layers, device=DEV, dtype=torch.bfloat16, seed=seed))
    return m


def _decode(m, prompts, n, use12):
    _lib_check(m.ctx.lib.pgv_llm_set_weight_stream(m.handle, use12))
    kv, nxt, lg = m.prefill(prompts, None, max(len(p) for p in prompts) + n + 4, want_logits=True)
    toks, logits = [nxt.clone()], [lg.clone()]
    for _ in range(n - 1):
        nxt, lg = m.decode_step(kv, nxt, want_logits=True)
        toks.append(nxt.clone()); logits.append(lg.clone())
    del kv
    return torch.stack(toks), torch.stack(logits)


def _lib_check(rc):
    from video_llava_amd import _lib
    _lib.check(rc, "pgv_llm_set_weight_stream")


def _prompts(B, vocab, seed):
    rng = np.random.default_rng(seed)
    return [[1] + rng.integers(3, vocab - 3, 20 + 7 * i).tolist() for i in range(B)]


@pytest.mark.parametrize("shape", ["7b", "13b"])
def test_model_decodes_identically_with_the_12bit_stream(ctx, shape):
    hidden, inter, heads = (4096, 11008, 32) if shape == "7b" else (5120, 13824, 40)
    vocab = 32003
    m = _model(hidden, inter, heads, 2, vocab, seed=21)
    lib = m.ctx.lib
    b16 = lib.pgv_llm_weight_stream_bytes(m.handle, 8)
    _lib_check(lib.pgv_llm_set_weight_stream(m.handle, 0))
    b16_off = lib.pgv_llm_weight_stream_bytes(m.handle, 8)
    _lib_check(lib.pgv_llm_set_weight_stream(m.handle, 1))
    assert 0.74 < b16 / b16_off < 0.76 and lib.pgv_llm_weight_stream_bytes(m.handle, 17) == b16_off
    for B in (3, 8, 12):
        prompts = _prompts(B, vocab, B)
        t12, l12 = _decode(m, prompts, 64, 1)
        t16, l16 = _decode(m, prompts, 64, 0)
        assert torch.equal(t12, t16) and torch.equal(l12, l16), (shape, B)
        assert torch.isfinite(l12).all()


def test_reloaded_weights_rebuild_the_12bit_copy(ctx):
    from video_llava_amd import _lib
    vocab, hidden, inter = 32003, 4096, 11008
    m = _model(hidden, inter, 32, 2, vocab, seed=5)
    prompts = _prompts(4, vocab, 9)
    _decode(m, prompts, 8, 1)                                         # graphs captured on the first copies
    g = torch.Generator(device=DEV).manual_seed(77)
    sd = {"model.layers.1.self_attn.q_proj.weight": (torch.randn(hidden, hidden, generator=g, device=DEV) * 0.03).to(torch.bfloat16),
          "model.layers.0.mlp.down_proj.weight": (torch.randn(hidden, inter, generator=g, device=DEV) * 0.01).to(torch.bfloat16),
          "model.layers.0.mlp.up_proj.weight": (torch.randn(inter, hidden, generator=g, device=DEV) * 0.05).to(torch.bfloat16)}
    for k, v in sd.items():
        _lib.check(m.ctx.lib.pgv_llm_load_tensor(m.handle, k.encode(), v.data_ptr(), _lib.dtype_code(v.dtype), 1, v.numel(), _lib.stream_ptr()), k)
    rows = (torch.randn(40, hidden, generator=g, device=DEV) * 0.04).to(torch.bfloat16)
    _lib.check(m.ctx.lib.pgv_llm_load_rows(m.handle, b"lm_head.weight", rows.data_ptr(), _lib.dtype_code(rows.dtype), 1, 100, 40, rows.numel(),
                                           _lib.stream_ptr()), "load_rows")
    t12, l12 = _decode(m, prompts, 16, 1)
    t16, l16 = _decode(m, prompts, 16, 0)
    assert torch.equal(t12, t16) and torch.equal(l12, l16)
    # ... and a vocabulary resize (new lm_head rows zeroed in both copies)
    m.resize_token_embeddings(vocab + 5)
    t12, l12 = _decode(m, prompts, 8, 1)
    t16, l16 = _decode(m, prompts, 8, 0)
    assert torch.equal(t12, t16) and torch.equal(l12, l16)
