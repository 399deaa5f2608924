"""oracle.clique_sim_ref — a plain numpy replay of `nfisam_simulate_clique` (csrc/clique_sim.hip), sample by sample.

Written from the kernel's contract (include/nfisam_hip.h, DESIGN.md §8 "the generator's contract"):

  generator   Philox4x32-10, counter = (sample, op index, 0x9E3779B9, 0x243F6A88), key = (seed & 0xffffffff, seed >> 32)
  uniforms    u_i = (float32(c_i >> 8) + 0.5f) * 2^-24 in float32: on (0, 1] (x + 0.5 rounds to even for x >= 2^23, so the
              largest value is exactly 1.0)
  normals     z0, z1 = Box-Muller of (u0, u1); z2 = sqrt(-2 log u2) cos(2 pi u3)
  bearings    phi = (2 u2 - 1) pi;  ADA_OBS and NH_OBS pick with u2, NH_RING picks with u3

The uniforms are rebuilt bit for bit, so every pick is exact; everything after them is a smooth function of known inputs
and runs in `dtype`.  `dtype=np.float64` is the reference; `dtype=np.float32` evaluates the same formulas with every
intermediate in numpy float32 and exists only to measure what float32 evaluation by itself costs (the tolerance of
tests/test_clique_sim_gpu.py is a multiple of the difference between the two).
"""
import numpy as np

MAX_OPS = 40
(COPY, PRIOR_SE2, REL_FWD, REL_BWD, REL_OBS, RING, RANGE_OBS, ADA_OBS, NH_RING, NH_OBS, PRIOR_R2, PRIOR_R2_RING,
 REL_R2_FWD, REL_R2_BWD, REL_R2_OBS) = range(1, 16)

# columns an op reads at a, reads at b and writes at c (0: the field is not used)
_WIDTHS = {PRIOR_SE2: (0, 0, 3), REL_FWD: (3, 0, 3), REL_BWD: (3, 0, 3), REL_OBS: (3, 3, 3), RING: (2, 0, 2),
           RANGE_OBS: (2, 2, 1), ADA_OBS: (2, 0, 1), NH_RING: (2, 0, 2), NH_OBS: (2, 2, 1), PRIOR_R2: (0, 0, 2),
           PRIOR_R2_RING: (0, 0, 2), REL_R2_FWD: (2, 0, 2), REL_R2_BWD: (2, 0, 2), REL_R2_OBS: (2, 2, 2)}

_M0, _M1 =np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter: four arrays (or ints) of 32-bit words, key: two -> four uint64
    arrays holding the 32-bit output words.  All arithmetic in uint64 (a 32 x 32 bit product fits)."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK for w in counter]
    k0, k1 = [np.uint64(int(w) & 0xFFFFFFFF) for w in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def unit_float32(words):
    """32-bit words -> float32 uniforms exactly as the kernel builds them: (float32(c >> 8) + 0.5f) * 2^-24, on (0, 1]."""
    w = np.asarray(words, dtype=np.uint64)
    u = (np.right_shift(w, np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and np.all(u > 0) and np.all(u <= 1)
    return u


def uniforms(seed, n, op_index):
    """The four float32 uniforms of samples 0..n-1 for op `op_index` under `seed`, exactly as the kernel builds them."""
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    words = philox4x32_10((np.arange(n, dtype=np.uint64), op_index, 0x9E3779B9, 0x243F6A88),
                          (seed & 0xFFFFFFFF, seed >> 32))
    return [unit_float32(w) for w in words]


class _Arith(object):
    """The kernel's formulas with every constant, input and intermediate in `dtype`."""

    def __init__(self, dtype, cancelling_exp=False):
        self.T = np.dtype(dtype).type
        self.pi, self.two_pi = self.T(np.pi), self.T(2 * np.pi)
        self.cancelling_exp = cancelling_exp      # the float32-cancelling (1 - cos w) / w, kept to show what it costs

    def wrap(self, t):
        r = np.fmod(t + self.pi, self.two_pi)
        r = np.where(r < 0, r + self.two_pi, r)
        return r - self.pi

    def draw(self, u):
        T = self.T
        u0, u1, u2, u3 = [x.astype(T) for x in u]
        r0, r1 = np.sqrt(T(-2) * np.log(u0)), np.sqrt(T(-2) * np.log(u2))
        return r0 * np.cos(self.two_pi * u1), r0 * np.sin(self.two_pi * u1), r1 * np.cos(self.two_pi * u3)

    def bearing(self, u2):
        return (self.T(2) * u2.astype(self.T) - self.T(1)) * self.pi

    def se2_exp(self, vx, vy, w):
        T = self.T
        small = np.abs(w) < T(1e-6)
        ws = np.where(small, T(1), w)                       # (keeps the unused lanes of the division finite)
        a = np.where(small, T(1), np.sin(ws) / ws)
        if self.cancelling_exp:
            b = (T(1) - np.cos(ws)) / ws
        else:
            s = np.sin(T(0.5) * ws)
            b = T(2) * s * s / ws
        b = np.where(small, T(0.5) * w, b)
        return a * vx - b * vy, b * vx + a * vy, self.wrap(w)

    def compose(self, A, B):
        c, s = np.cos(A[2]), np.sin(A[2])
        return A[0] + c * B[0] - s * B[1], A[1] + s * B[0] + c * B[1], self.wrap(A[2] + B[2])

    def inverse(self, A):
        c, s = np.cos(A[2]), np.sin(A[2])
        return -(c * A[0] + s * A[1]), -(-s * A[0] + c * A[1]), self.wrap(-A[2])

    def noise_pose(self, L, z):
        return self.se2_exp(L[0] * z[0], L[1] * z[0] + L[2] * z[1], L[3] * z[0] + L[4] * z[1] + L[5] * z[2])


def replay(ops, n, D_out, D_total, seed, sources, dtype=np.float64, _cancelling_exp=False):
    """What `nfisam_simulate_clique(ops, n, D_out, D_total, seed)` must return: [n, D_out] in `dtype`.

    ops      `nfisam_hip.SimOp`s, or plain records with the fields code, a, b, c, k, cand, p, src
    sources  {src of a COPY op: its host array [n, a]} (the row-major array the device pointer `src` stands for)
    """
    n, D_out, D_total = int(n), int(D_out), int(D_total)
    assert 1 <= len(ops) <= MAX_OPS and n >= 1 and 1 <= D_out <= D_total
    ar = _Arith(dtype, _cancelling_exp)
    T = ar.T
    X = np.zeros((D_total, n), dtype=T)

    def pose(c):
        return X[c], X[c + 1], X[c + 2]

    def put(c, vals):
        for j, v in enumerate(vals):
            X[c + j] = v
            assert X[c + j].dtype == T and np.asarray(v).dtype == T

    for o, op in enumerate(ops):
        code, a, b, c, k = int(op.code), int(op.a), int(op.b), int(op.c), int(op.k)
        p32 = np.array([np.float32(v) for v in op.p], dtype=np.float32)          # the ABI stores p[] in float32
        p = p32.astype(T)
        if code == COPY:
            src = np.asarray(sources[int(op.src)]).astype(np.float32)              # ... and the messages too
            assert src.shape == (n, a) and 0 <= b and k >= 1 and b + k <= a and 0 <= c and c + k <= D_total
            put(c, [src[:, b + j].astype(T) for j in range(k)])
            continue
        assert PRIOR_SE2 <= code <= REL_R2_OBS
        wa, wb, wc = _WIDTHS[code]
        reads = [(a, wa), (b, wb), (c, wc)] + ([(int(op.cand[j]), 2) for j in range(k)] if code == ADA_OBS else [])
        assert all(w == 0 or (0 <= first and first + w <= D_total) for first, w in reads), (o, code, reads)
        u = uniforms(seed, n, o)
        z = ar.draw(u)
        if code in (PRIOR_SE2, REL_FWD, REL_BWD):
            x = ar.compose((p[0], p[1], p[2]), ar.noise_pose(p[3:9], z))
            if code == REL_FWD:
                x = ar.compose(pose(a), x)
            elif code == REL_BWD:
                x = ar.compose(pose(a), ar.inverse(x))
            put(c, x)
        elif code == REL_OBS:
            put(c, ar.compose(ar.compose(ar.inverse(pose(a)), pose(b)), ar.noise_pose(p[3:9], z)))
        elif code in (RING, NH_RING, PRIOR_R2_RING):
            if code == RING:
                cx, cy, rad = X[a], X[a + 1], p[0] + p[1] * z[0]
            elif code == NH_RING:
                sig = np.where(u[3] < p32[3], p[1], p[2])
                cx, cy, rad = X[a], X[a + 1], p[0] + sig * z[0]
            else:
                cx, cy, rad = p[0], p[1], p[2] + p[3] * z[0]
            phi = ar.bearing(u[2])
            put(c, [cx + rad * np.cos(phi), cy + rad * np.sin(phi)])
        elif code in (RANGE_OBS, NH_OBS, ADA_OBS):
            if code == ADA_OBS:
                assert 1 <= k <= 4
                pick = np.full(n, k - 1)
                for j in range(k - 2, -1, -1):
                    pick = np.where(u[2] < p32[j], j, pick)
                cand = np.array([int(op.cand[j]) for j in range(k)])[pick]
                tx, ty, sig = X[cand, np.arange(n)], X[cand + 1, np.arange(n)], p[4]
            else:
                tx, ty = X[b], X[b + 1]
                sig = p[0] if code == RANGE_OBS else np.where(u[2] < p32[2], p[0], p[1])
            dx, dy = tx - X[a], ty - X[a + 1]
            put(c, [np.sqrt(dx * dx + dy * dy) + sig * z[0]])
        elif code == PRIOR_R2:
            put(c, [p[0] + p[2] * z[0], p[1] + p[3] * z[0] + p[4] * z[1]])
        elif code in (REL_R2_FWD, REL_R2_BWD):
            sg = T(1) if code == REL_R2_FWD else T(-1)
            put(c, [X[a] + sg * (p[0] + p[2] * z[0]), X[a + 1] + sg * (p[1] + (p[3] * z[0] + p[4] * z[1]))])
        else:                                                                       # REL_R2_OBS
            put(c, [X[b] - X[a] + p[2] * z[0], X[b + 1] - X[a + 1] + p[3] * z[0] + p[4] * z[1]])
    return np.ascontiguousarray(X[:D_out].T)
