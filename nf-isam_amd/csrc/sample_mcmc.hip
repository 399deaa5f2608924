// sample_mcmc.hip — Metropolis-corrected moves of the posterior samples: the Langevin (or random-walk) proposal and the
// accept / reject step of n parallel chains.
//
// Every other unit over the sample matrix grades, describes or pushes the draw; this one makes it a Markov chain whose
// stationary distribution is the target itself.  A chain is a column of the column-major float32 matrix Xt[x_rows][n] (the tree
// walk's St); its score is the same column of the float64 matrix Gx[x_rows][n] that nfisam_factor_graph_score writes.  With a
// step length h_r per row, in the row's own unit (0 freezes the row), the MALA proposal is
//     y_r = x_r + (h_r^2 / 2) g_r + h_r z_r,        z_r ~ N(0, 1)
// (no Gx: the random walk y_r = x_r + h_r z_r), wrapped into [-pi, pi) where wrap[r] is set and rounded to float32 by the rule
// of the SVGD step: a wrapped value that rounds to +-float32(pi) becomes the float32 just inside -pi.  The accept step forms
//     log alpha = (lp_y - lp_x) + sum_{r: h_r > 0} [ -1/2 ((d_r - (h_r^2/2) gy_r) / h_r)^2 + 1/2 ((-d_r - (h_r^2/2) gx_r) / h_r)^2 ]
// with d_r = (double)x_r - (double)y_r, the float64 difference of the float32 values ACTUALLY STORED (the ratio is exact for
// the move that was made), brought into [-pi, pi] as sign(d) wrap(|d|) on wrapped rows: the nearest-image form of the wrapped
// normal, -d_r being the same bits with the other sign.  Without Gx / Gy the sum is absent (a symmetric proposal: the random
// walk, or -- with lp = log p - log q -- an independence step).  The chain accepts iff log(u) < log alpha; a NaN log alpha
// rejects, lp_y = -inf rejects, lp_x = -inf with a finite lp_y accepts.  On accept column i of Yt / Gy / lp_y replaces column i
// of Xt / Gx / lp_x; a rejected chain keeps every bit.
//
// THE GENERATOR IS A CONTRACT.  Philox4x32-10 with the constants of clique_sim.hip, restated here; key
// (seed & 0xffffffff, seed >> 32); counter (chain i, row r >> 2, step t, tag): tag 0 the normals, tag 1 the accept uniform
// (row word 0).  u = (word + 0.5) 2^-32 in float64, exactly representable and strictly inside (0, 1).  The four normals of a
// counter block are Box-Muller of (u0, u1) -> rows 4g, 4g + 1 (cos, sin) and of (u2, u3) -> rows 4g + 2, 4g + 3.  A chain's
// draws depend on (seed, i, r, t) alone: never on n, the tile or the launch shape.
//
// Numerics: the contract of sample_common.h -- float32 points in, every difference, product, transcendental and sum float64.
//
// LAUNCHES, no float atomics.  Propose: one launch, a wave per (64 chains, 4 rows = one counter block); h and wrap of the
// block's rows are wave-uniform and read as scalars.  Accept: two launches.  (1) grid (tiles of 64 chains, slabs of SLAB rows),
// 256 threads: wave w adds the terms of rows slab * SLAB + w * SLAB / 4 ... ascending, the four waves' sums are parked in LDS
// and combined by waves_in_order, one store to scratch[slab][i]; the block of slab 0 also parks lp_y - lp_x behind the slabs.
// (2) the same tiles over groups of rows: every block adds the slabs of its 64 chains in slab order, decides, and copies its rows
// of the accepted columns; the block of group 0 writes log_alpha, accepted and lp_x.  (2) reads lp_x nowhere, which is why (1)
// parks the difference: no block can see another's update.  The order of the sum depends on x_rows alone, so a chain's log_alpha
// is the same bits at any n, in any tile, on every call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sample_common.h"

namespace {

using namespace sample_common;

constexpr int TILE = 64;          // chains per block: one per lane
constexpr int SLAB = 32;          // rows per block of the first accept launch: 8 per wave
constexpr int RPW = SLAB / 4;     // rows per wave
constexpr int MAX_GROUPS = 128;   // blocks along the rows in the second accept launch (each re-adds the slabs of its chains)
static_assert(SLAB % 4 == 0, "the four waves share a slab");

// ---- Philox4x32-10 (Salmon et al., SC'11), the constants of clique_sim.hip ---------------------------------------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// the four float64 uniforms of counter (chain, word, t, tag) under `seed`: (word + 0.5) 2^-32, inside (0, 1) exactly
__device__ __forceinline__ void philox_uniforms(unsigned long long seed, uint32_t chain, uint32_t word, uint32_t t, uint32_t tag,
                                                double (&u)[4]) {
    uint32_t c[4] = {chain, word, t, tag};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = ((double)c[k] + 0.5) * (1.0 / 4294967296.0);
}

// sign(d) wrap(|d|): -d gives the same bits with the other sign (sample_pairs.h's signed_wrap; this unit includes sample_common.h alone)
__device__ __forceinline__ double signed_wrap(double d) {
    const double m = wrap_pi_near(fabs(d));
    return (d < 0.0) ? -m : m;
}

// the SVGD step's rounding of a moved coordinate: a wrapped value that rounds to +-float32(pi) lies outside [-pi, pi)
__device__ __forceinline__ float round_point(double y, bool wrapped) {
    float f = (float)y;
    if (wrapped) {
        f = (float)wrap_pi(y);
        if (!((double)f < PI && (double)f >= -PI)) f = -3.1415925f;
        if (isnan(y)) f = (float)y;
    }
    return f;
}

// grid (tiles of 64 chains, min(groups of 16 rows, 65535)); 256 threads: wave w of block (bx, by) takes the counter blocks
// 4 by + w, + 4 gridDim.y, ... of the chains 64 bx ... (a counter block = 4 rows)
__global__ void __launch_bounds__(256) mcmc_propose_kernel(const float* __restrict__ Xt, const double* __restrict__ Gx,
                                                           float* __restrict__ Yt, int x_rows, int n, const double* __restrict__ h,
                                                           const uint8_t* __restrict__ wrap, unsigned long long seed, uint32_t t) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // provably wave-uniform: h and wrap go through scalar loads
    const int i = blockIdx.x * TILE + lane;
    if (i >= n) return;
    const int groups = (x_rows + 3) >> 2;
    for (int g = 4 * (int)blockIdx.y + w; g < groups; g += 4 * (int)gridDim.y) {
        const int r0 = 4 * g, cnt = min(4, x_rows - r0);
        double hr[4];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hr[k] = k < cnt ? h[r0 + k] : 0.0;
            any = any || hr[k] != 0.0;
        }
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        if (any) {                                                     // (wave-uniform: a frozen block draws nothing)
            double u[4];
            philox_uniforms(seed, (uint32_t)i, (uint32_t)g, t, 0u, u);
            const double ra = sqrt(-2.0 * log(u[0])), rb = sqrt(-2.0 * log(u[2]));
            const double ta = TWO_PI * u[1], tb = TWO_PI * u[3];
            z[0] = ra * cos(ta); z[1] = ra * sin(ta);
            z[2] = rb * cos(tb); z[3] = rb * sin(tb);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < cnt) {
                const size_t at = (size_t)(r0 + k) * (size_t)n + (size_t)i;
                const float x = Xt[at];
                float y = x;                                           // h == 0: the bits of Xt
                if (hr[k] != 0.0) {
                    double v = (double)x + hr[k] * z[k];
                    if (Gx != nullptr) v += (0.5 * hr[k] * hr[k]) * Gx[at];
                    y = round_point(v, wrap != nullptr && wrap[r0 + k] != 0);
                }
                Yt[at] = y;
            }
        }
    }
}

// grid (tiles of 64 chains, slabs); 256 threads.  Gx == nullptr: one slab's worth of blocks, the difference lp_y - lp_x alone
__global__ void __launch_bounds__(256) mcmc_partial_kernel(const float* __restrict__ Xt, const float* __restrict__ Yt,
                                                           const double* __restrict__ Gx, const double* __restrict__ Gy,
                                                           const double* __restrict__ lp_x, const double* __restrict__ lp_y,
                                                           int x_rows, int n, int n_slabs, const double* __restrict__ h,
                                                           const uint8_t* __restrict__ wrap, double* __restrict__ scratch) {
    __shared__ double wsum[4][TILE];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * TILE + lane, slab = blockIdx.y;
    const size_t ic = (size_t)(i < n ? i : n - 1);
    if (slab == 0 && w == 0 && i < n) scratch[(size_t)n_slabs * (size_t)n + (size_t)i] = lp_y[i] - lp_x[i];
    if (Gx == nullptr) return;                                         // (uniform over the launch)
    double s = 0.0;
    const int r0 = slab * SLAB + w * RPW;
#pragma unroll
    for (int k = 0; k < RPW; ++k) {                                    // the thread's rows, ascending
        const int r = r0 + k;
        if (r < x_rows) {
            const double hr = h[r];
            if (hr > 0.0) {
                const size_t at = (size_t)r * (size_t)n + ic;
                double d = (double)Xt[at] - (double)Yt[at];
                if (wrap != nullptr && wrap[r] != 0) d = signed_wrap(d);
                const double a = 0.5 * hr * hr;
                const double rev = (d - a * Gy[at]) / hr, fwd = (-d - a * Gx[at]) / hr;
                s += 0.5 * (fwd * fwd) - 0.5 * (rev * rev);
            }
        }
    }
    wsum[w][lane] = s;
    __syncthreads();
    if (w == 0 && i < n) {
        const double p4[4] = {wsum[0][lane], wsum[1][lane], wsum[2][lane], wsum[3][lane]};
        scratch[(size_t)slab * (size_t)n + (size_t)i] = waves_in_order(p4);
    }
}

// grid (tiles of 64 chains, groups of rows); 256 threads: every block decides for its 64 chains (the slabs in slab order), then
// wave w copies the rows 4 q + w of its run of rows for the accepted ones; the block of group 0 writes the per-chain results
__global__ void __launch_bounds__(256) mcmc_decide_kernel(float* __restrict__ Xt, const float* __restrict__ Yt,
                                                          double* __restrict__ Gx, const double* __restrict__ Gy,
                                                          double* __restrict__ lp_x, const double* __restrict__ lp_y, int x_rows, int n,
                                                          int n_slabs, int sum_slabs, int rows_per_group, unsigned long long seed,
                                                          uint32_t t, const double* __restrict__ scratch,
                                                          double* __restrict__ log_alpha, uint8_t* __restrict__ accepted) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * TILE + lane;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < sum_slabs; ++k) s += scratch[(size_t)k * (size_t)n + (size_t)i];
    const double lpy = lp_y[i];
    const double la = scratch[(size_t)n_slabs * (size_t)n + (size_t)i] + s;
    double u[4];
    philox_uniforms(seed, (uint32_t)i, 0u, t, 1u, u);
    // NaN compares false: a NaN log alpha rejects; lp_y = -inf gives -inf or NaN; lp_x = -inf with a finite lp_y gives +inf
    const bool acc = log(u[0]) < la && lpy != -INFINITY;
    if (blockIdx.y == 0 && w == 0) {
        log_alpha[i] = la;
        accepted[i] = acc ? 1 : 0;
        if (acc) lp_x[i] = lpy;
    }
    if (!acc) return;
    const int r_begin = (int)blockIdx.y * rows_per_group, r_end = min(x_rows, r_begin + rows_per_group);
    for (int r = r_begin + w; r < r_end; r += 4) {
        const size_t at = (size_t)r * (size_t)n + (size_t)i;
        Xt[at] = Yt[at];
        if (Gx != nullptr) Gx[at] = Gy[at];
    }
}

inline bool shape(int x_rows, int n, unsigned* tiles, int* n_slabs) {
    if (x_rows < 1 || n < 1) return false;
    const long long t = ((long long)n + TILE - 1) / TILE;
    if (t > 65535) return false;                                       // n <= 65535 * 64
    *tiles = (unsigned)t;
    *n_slabs = (int)(((long long)x_rows + SLAB - 1) / SLAB);
    return *n_slabs <= 65535;                                          // the accept step's second dimension: x_rows <= 65535 * 32
}

}  // namespace

extern "C" int nfisam_sample_propose(const float* Xt, const double* Gx, float* Yt, int x_rows, int n, const double* h,
                                     const uint8_t* wrap, uint64_t seed, uint32_t t, nfisam_stream_t stream) {
    if (Xt == nullptr || Yt == nullptr || h == nullptr) return NFISAM_ERR_ARG;
    unsigned tiles;
    int n_slabs;
    if (!shape(x_rows, n, &tiles, &n_slabs)) return NFISAM_ERR_ARG;
    const long long blocks = (((long long)x_rows + 3) / 4 + 3) / 4;      // four counter blocks (16 rows) per group of 4 waves
    hipLaunchKernelGGL(mcmc_propose_kernel, dim3(tiles, (unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0,
                       (hipStream_t)stream, Xt, Gx, Yt, x_rows, n, h, wrap, (unsigned long long)seed, t);
    return launch_status(hipGetLastError());
}

extern "C" size_t nfisam_sample_accept_scratch_count(int x_rows, int n) {
    unsigned tiles;
    int n_slabs;
    if (!shape(x_rows, n, &tiles, &n_slabs)) return 0;
    return ((size_t)n_slabs + 1) * (size_t)n;                            // one partial per (slab, chain) + lp_y - lp_x
}

extern "C" int nfisam_sample_accept(float* Xt, const float* Yt, double* Gx, const double* Gy, double* lp_x, const double* lp_y,
                                    int x_rows, int n, const double* h, const uint8_t* wrap, uint64_t seed, uint32_t t,
                                    double* log_alpha, uint8_t* accepted, double* scratch, nfisam_stream_t stream) {
    if (Xt == nullptr || Yt == nullptr || lp_x == nullptr || lp_y == nullptr || h == nullptr || log_alpha == nullptr ||
        accepted == nullptr || scratch == nullptr)
        return NFISAM_ERR_ARG;
    if ((Gx == nullptr) != (Gy == nullptr)) return NFISAM_ERR_ARG;
    unsigned tiles;
    int n_slabs;
    if (!shape(x_rows, n, &tiles, &n_slabs)) return NFISAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const bool drift = Gx != nullptr;
    hipLaunchKernelGGL(mcmc_partial_kernel, dim3(tiles, drift ? (unsigned)n_slabs : 1u), dim3(256), 0, s, Xt, Yt, Gx, Gy, lp_x, lp_y,
                       x_rows, n, n_slabs, h, wrap, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const int per = (int)((((long long)n_slabs + MAX_GROUPS - 1) / MAX_GROUPS) * SLAB);   // whole slabs, at most MAX_GROUPS groups
        const unsigned groups = (unsigned)(((long long)x_rows + per - 1) / per);
        hipLaunchKernelGGL(mcmc_decide_kernel, dim3(tiles, groups), dim3(256), 0, s, Xt, Yt, Gx, Gy, lp_x, lp_y, x_rows, n, n_slabs,
                           drift ? n_slabs : 0, per, (unsigned long long)seed, t, scratch, log_alpha, accepted);
        e = hipGetLastError();
    }
    return launch_status(e);
}
