"""numpy restatement of the device generator, written from DESIGN.md section 3 "Device randomness"
(not from the kernels): Philox4x32-10, the noise blocks and the schedule permutations.

    philox4x32_10(counter[..., 4], key[..., 2]) -> words[..., 4]
    noise(seed, pos, n_steps, N, n_agents, A, dtype) -> [n_steps, N, n_agents, A]
    permutation(seed, draw, policy, array, n) -> int32 [n]
    schedule(seed, draw, policy, R, nb, epochs) -> (shuffle [R], perm [epochs, nb])
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
FEISTEL_ROUNDS = 4


def philox4x32_10(counter, key):
    c = [np.asarray(counter[..., i], np.uint64) & MASK32 for i in range(4)]
    k0 = np.asarray(key[..., 0], np.uint64) & MASK32
    k1 = np.asarray(key[..., 1], np.uint64) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, -1).astype(np.uint32)


def _split64(x):
    x = int(x) & ((1 << 64) - 1)
    return x & MASK32, x >> 32


def noise_words(seed, pos, n_steps, N, B):
    """The Philox words of the noise blocks: uint32 [n_steps, N, B, 4]; counter = (s lo, s hi, e, b)
    with s = pos + step the absolute step, key = (seed lo, seed hi)."""
    s = (np.arange(n_steps, dtype=np.uint64) + np.uint64(int(pos) & ((1 << 64) - 1)))[:, None, None]
    e = np.arange(N, dtype=np.uint64)[None, :, None]
    b = np.arange(B, dtype=np.uint64)[None, None, :]
    shape = (n_steps, N, B)
    ctr = np.stack([np.broadcast_to(s & np.uint64(MASK32), shape), np.broadcast_to(s >> np.uint64(32), shape),
                    np.broadcast_to(e, shape), np.broadcast_to(b, shape)], -1)
    k = np.array(_split64(seed), np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(k, shape + (2,)))


def normals_from_words(w, dtype=np.float64):
    """Box-Muller on (w0, w1) and (w2, w3): u = ((w >> 8) + 0.5) 2^-24, r = sqrt(-2 ln u1),
    (r cos 2 pi u2, r sin 2 pi u2); every operation in `dtype`."""
    f = dtype
    u = ((w >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    out = np.empty(w.shape, f)
    for a in (0, 2):
        r = np.sqrt(f(-2.0) * np.log(u[..., a]))
        ang = f(2.0 * np.pi) * u[..., a + 1]
        out[..., a] = r * np.cos(ang)
        out[..., a + 1] = r * np.sin(ang)
    return out


def noise(seed, pos, n_steps, N, n_agents, A, dtype=np.float64):
    comps = n_agents * A
    assert comps % 4 == 0
    w = noise_words(seed, pos, n_steps, N, comps // 4)
    return normals_from_words(w, dtype).reshape(n_steps, N, n_agents, A)


def half_bits(n):
    """The smallest h >= 1 with 4^h >= n."""
    h = 1
    while 4 ** h < n:
        h += 1
    return h


def _feistel(v, seed, d, tag, h):
    """One pass of the network over the values v; d: the draw index of every value (uint64)."""
    mask = np.uint64((1 << h) - 1)
    L, R = v >> np.uint64(h), v & mask
    d0, d1 = d & np.uint64(MASK32), d >> np.uint64(32)
    k = np.broadcast_to(np.array(_split64(seed), np.uint64), v.shape + (2,))
    for r in range(FEISTEL_ROUNDS):
        ctr = np.stack([R, d0, d1, np.full_like(R, tag | (r << 24))], -1)
        f = philox4x32_10(ctr, k)[..., 0].astype(np.uint64)
        L, R = R, L ^ (f & mask)
    return (L << np.uint64(h)) | R


def permutation(seed, draw, policy, array, n):
    """Array `array` (0: the shuffle, 1 + e: epoch e's perm) of `policy` in draw `draw`: element i is
    i sent through the 4-round Feistel network over 2 h bits, again while the value is >= n.
    int32 [n]; with an array of draw indices, one row per draw."""
    tag = 0x80000000 | (policy << 28) | array
    h = half_bits(n)
    draws = np.atleast_1d(np.asarray(draw, np.uint64))
    v = np.broadcast_to(np.arange(n, dtype=np.uint64), (draws.size, n)).copy()
    d = np.broadcast_to(draws[:, None], v.shape)
    todo = np.ones(v.shape, bool)
    while todo.any():
        v[todo] = _feistel(v[todo], seed, d[todo], tag, h)
        todo = v >= n
    v = v.astype(np.int32)
    return v if np.ndim(draw) else v[0]


def schedule(seed, draw, policy, R, nb, epochs):
    shuffle = permutation(seed, draw, policy, 0, R)
    perm = np.stack([permutation(seed, draw, policy, 1 + e, nb) for e in range(epochs)])
    return shuffle, perm
