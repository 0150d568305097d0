"""numpy twin of the lossless 12-bit weight stream (video_llava_amd/csrc/w12.h): encoder and decoder on raw bf16 bit patterns.

encode(bits [N, K] uint16) -> (buffer uint8 of pgv_w12_bytes(N, K), exception counts per 16-row block); decode(buffer, N, K) -> bits.
The buffer is byte for byte what pgv_encode_w12_blocked writes whenever every row block has at most 64 exceptions."""
import numpy as np

MAX_EXC = 64
NO_EXC = 0xFFFFFFFF


def nbytes(N, K):
    return N * K * 3 // 2 + (N // 16) * MAX_EXC * 4 + N


def row_bases(bits):
    """Per row: the first b whose window [b - 7, b] of 7-bit exponents holds the most weights."""
    N = bits.shape[0]
    e7 = ((bits >> 8) & 0x7F).astype(np.int64)
    hist = np.zeros((N, 128), np.int64)
    np.add.at(hist, (np.repeat(np.arange(N), bits.shape[1]), e7.ravel()), 1)
    c = np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(hist, 1)], 1)        # c[:, b + 1] = sum hist[:, :b + 1]
    b = np.arange(128)
    win = c[:, b + 1] - c[:, np.maximum(b - 7, 0)]
    return np.argmax(win, 1).astype(np.int64)


def _to_units(a, N, K):
    """[N, K] -> [N/16, G, 64 lanes, 2 k-blocks, 8]: lane (k % 32) / 8 * 16 + n % 16, k-block (k / 32) % 2, element k % 8."""
    return a.reshape(N // 16, 16, K // 64, 2, 4, 8).transpose(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 64, 64, 2, 8)


def _from_units(u, N, K):
    return u.reshape(N // 16, K // 64, 4, 16, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(N, K)


def encode(bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    N, K = bits.shape
    assert N % 16 == 0 and K % 64 == 0
    G = K // 64
    base = row_bases(bits)
    hb = (bits >> 8).astype(np.int64)
    d = base[:, None] - (hb & 0x7F)
    ok = (d >= 0) & (d <= 7)
    code = np.where(ok, ((hb >> 7) << 3) | np.where(ok, d, 0), 0)
    lo_u = _to_units((bits & 0xFF).astype(np.uint8), N, K)                      # [R, G, 64, 2, 8]
    c_u = _to_units(code.astype(np.uint8), N, K)
    packed = (c_u[..., :4] | (c_u[..., 4:] << 4)).astype(np.uint8)               # [R, G, 64, 2, 4]
    units = np.concatenate([lo_u.reshape(N // 16, G, 1024), packed.reshape(N // 16, G, 512)], 2)
    # exceptions: group << 18 | lane << 12 | byte << 8 | high byte
    exc_u = _to_units(~ok, N, K)
    hb_u = _to_units(hb, N, K)
    g_i, l_i, h_i, e_i = np.meshgrid(np.arange(G), np.arange(64), np.arange(2), np.arange(8), indexing="ij")
    key = (g_i.astype(np.int64) << 18) | (l_i << 12) | ((h_i * 8 + e_i) << 8)
    exc = np.full((N // 16, MAX_EXC), NO_EXC, np.uint32)
    counts = np.zeros(N // 16, np.int64)
    for rb in range(N // 16):
        m = exc_u[rb]
        ent = np.sort((key[m] | hb_u[rb][m]).astype(np.uint32))
        counts[rb] = ent.size
        exc[rb, :min(ent.size, MAX_EXC)] = ent[:MAX_EXC]
    buf = np.concatenate([units.ravel(), exc.view(np.uint8).ravel(), base.astype(np.uint8)])
    assert buf.size == nbytes(N, K)
    return buf, counts


def decode(buf, N, K):
    G = K // 64
    nu = N * K * 3 // 2
    units = buf[:nu].reshape(N // 16, G, 1536)
    exc = buf[nu:nu + (N // 16) * MAX_EXC * 4].view(np.uint32).reshape(N // 16, MAX_EXC)
    base = buf[nu + (N // 16) * MAX_EXC * 4:].astype(np.int64)
    lo = units[..., :1024].reshape(N // 16, G, 64, 2, 8).astype(np.int64)
    pk = units[..., 1024:].reshape(N // 16, G, 64, 2, 4).astype(np.int64)
    code = np.concatenate([pk & 0xF, pk >> 4], -1)                               # [R, G, 64, 2, 8]
    lane_row = np.arange(64) % 16
    b = base.reshape(N // 16, 16)[:, None, lane_row, None, None]                # row base of every lane
    hi = (b - (code & 7)) | ((code & 8) << 4)
    for rb in range(N // 16):
        for e in exc[rb]:
            if e == NO_EXC:
                continue
            e = int(e)
            byte = (e >> 8) & 15
            hi[rb, e >> 18, (e >> 12) & 63, byte >> 3, byte & 7] = e & 0xFF
    return _from_units(((hi << 8) | lo).astype(np.uint16), N, K)


def bf16_bits(t):
    """torch bf16 tensor -> numpy uint16 bit patterns."""
    import torch
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)
