// sample_chains.hip — streaming diagnostics of n parallel chains: split-R-hat, the blocking estimate of the integrated
// autocorrelation time and the within-chain variance of every coordinate, without keeping the chains' history.
//
// sample_mcmc.hip moves the chains; this unit says whether they have mixed.  A chain is a column of the column-major float32
// matrix Xt[x_rows][n]; its history (rows x chains x steps) cannot be kept and the matrix never leaves the device, so between two
// steps ONE launch folds the current state into float64 accumulators per (row, chain), and after the last step ONE launch turns
// the accumulators into per-row statistics.  T recorded states, t = 0 ... T - 1, T even; the recorded value of row r, chain i is
// the deviation from a per-row centre,
//     v = (double)Xt[r][i] - center[r],        wrap_pi(...) of it where wrap[r] is set
// (the centre keeps the sums well conditioned: coordinates reach 100 m with spreads of centimetres).
//
// THE STATE, slot-major [slot][row][chain] (a lane per chain reads and writes coalesced), zeros before t = 0:
//     slot 0, 1: A1[w] = sum v          slot 2, 3: A2[w] = sum v^2          w = 0 for t < T / 2, w = 1 for t >= T / 2
//     slot 4 + 3 (l - 1) + {0, 1, 2}: P_l, R_l, Q_l of blocking level l = 1 ... levels - 1 (Flyvbjerg & Petersen 1989): the
//     pending half of a block of 2^l consecutive values, R_l = sum_j b_lj and Q_l = sum_j b_lj^2 over the complete blocks'
//     means b_lj.  Level 0 is the halves added up.
// THE FOLD at index t: A1[w] += v, A2[w] += v^2, then carry = v and for l = 1 ... levels - 1: bit l - 1 of t clear -> P_l =
// carry, stop; set -> carry = (P_l + carry) / 2, R_l += carry, Q_l += carry^2, go on.  The depth depends on t alone: control
// flow is uniform over the launch, about two level updates per step amortised.
//
// THE FINISH of row r over its n chains, with m_l = T >> l and s2_li = (Q_l - R_l^2 / m_l) / (m_l - 1):
//     mean   = center + sum_i (A1[0] + A1[1]) / (n T)                                    (wrapped on a circular row)
//     within = mean_i s2_0i
//     tau[l] = 2^l mean_i s2_li / mean_i s2_0i                                           (tau[0] = 1 by construction)
//     rhat   = sqrt(((L - 1) / L W + B / L) / W), over the 2 n half-chains of length L = T / 2 (BDA3 11.4): mu_k = A1 / L,
//              s2_k = (A2 - A1^2 / L) / (L - 1), W = mean_k s2_k, B / L = sum_k (mu_k - mu_bar)^2 / (2 n - 1) in two passes;
//              NaN for T < 4, and NaN where W = 0 and B = 0 (a row without spread): 0 / 0, no special case.
//
// Numerics: the contract of sample_common.h -- float32 points in, every difference, product and sum float64.
//
// LAUNCHES, no float atomics.  Record: grid (tiles of 64 chains, groups of 4 rows), 256 threads; a wave takes one row at a
// time, center[r] and wrap[r] are wave-uniform and read as scalars; elementwise, so every call gives the same bits at any n,
// in any tile, alone or inside a taller matrix.  Finish: one block of 256 threads per row; a thread adds its chains ascending
// (i = thread, thread + 256, ...), then wave_sum, then waves_in_order: the order depends on n alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sample_common.h"

namespace {

using namespace sample_common;

constexpr int TILE = 64;          // chains per block of the record launch: one per lane
constexpr int MAX_LEVELS = 16;    // NFISAM_CHAIN_MAX_LEVELS

// grid (tiles of 64 chains, min(groups of 4 rows, 65535)); 256 threads: wave w of block (bx, by) takes the rows 4 by + w,
// + 4 gridDim.y, ... of the chains 64 bx ...; `half` = (t >= T / 2)
__global__ void __launch_bounds__(256) chain_record_kernel(const float* __restrict__ Xt, double* __restrict__ state, int x_rows,
                                                           int n, int levels, const double* __restrict__ center,
                                                           const uint8_t* __restrict__ wrap, uint32_t t, int half) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // provably wave-uniform: center and wrap go through scalar loads
    const int i = blockIdx.x * TILE + lane;
    if (i >= n) return;
    const size_t plane = (size_t)x_rows * (size_t)n;
    for (int r = 4 * (int)blockIdx.y + w; r < x_rows; r += 4 * (int)gridDim.y) {
        const size_t at = (size_t)r * (size_t)n + (size_t)i;
        double* a1 = state + (size_t)half * plane + at;
        double* a2 = state + (size_t)(2 + half) * plane + at;
        const double s1 = *a1, s2 = *a2;                               // (the loads go out together, ahead of the stores)
        double v = (double)Xt[at] - (center != nullptr ? center[r] : 0.0);
        if (wrap != nullptr && wrap[r] != 0) v = wrap_pi(v);
        *a1 = s1 + v;
        *a2 = s2 + v * v;
        double carry = v;
        for (int l = 1; l < levels; ++l) {                             // (uniform over the launch: the depth depends on t alone)
            double* p = state + (size_t)(4 + 3 * (l - 1)) * plane + at;
            if (((t >> (l - 1)) & 1u) == 0u) {
                *p = carry;
                break;
            }
            const double pend = *p, rs = p[plane], qs = p[2 * plane];
            carry = 0.5 * (pend + carry);
            p[plane] = rs + carry;
            p[2 * plane] = qs + carry * carry;
        }
    }
}

// the sum of one value per thread over the block, in every thread: wave_sum, then the four waves in order
__device__ __forceinline__ double block_sum(double v, double* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = waves_in_order(part);
    __syncthreads();
    return s;
}

// grid (rows); 256 threads: block r finishes row r
__global__ void __launch_bounds__(256) chain_finish_kernel(const double* __restrict__ state, int x_rows, int n, int levels, uint32_t T,
                                                           const double* __restrict__ center, const uint8_t* __restrict__ wrap,
                                                           double* __restrict__ mean, double* __restrict__ within,
                                                           double* __restrict__ rhat, double* __restrict__ tau) {
    __shared__ double part[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t plane = (size_t)x_rows * (size_t)n;
    const double* base = state + (size_t)r * (size_t)n;
    const double Td = (double)T, L = (double)(T / 2);
    double sv = 0.0, sm = 0.0, sw = 0.0, s0 = 0.0;
    for (int i = tid; i < n; i += 256) {                               // the thread's chains, ascending; a chain's halves in order
        const double a10 = base[i], a11 = base[plane + i], a20 = base[2 * plane + i], a21 = base[3 * plane + i];
        const double r0 = a10 + a11, q0 = a20 + a21;
        sv += r0;
        sm += a10 / L;
        sm += a11 / L;
        sw += (a20 - a10 * a10 / L) / (L - 1.0);
        sw += (a21 - a11 * a11 / L) / (L - 1.0);
        s0 += (q0 - r0 * r0 / Td) / (Td - 1.0);
    }
    sv = block_sum(sv, part);
    sm = block_sum(sm, part);
    sw = block_sum(sw, part);
    s0 = block_sum(s0, part);
    const double halves = 2.0 * (double)n;
    const double mu_bar = sm / halves;
    double sb = 0.0;
    for (int i = tid; i < n; i += 256) {                               // the second pass of the variance of the half-chain means
        const double d0 = base[i] / L - mu_bar, d1 = base[plane + i] / L - mu_bar;
        sb += d0 * d0;
        sb += d1 * d1;
    }
    sb = block_sum(sb, part);
    const double var0 = s0 / (double)n;
    if (tid == 0) {
        double m = (center != nullptr ? center[r] : 0.0) + sv / ((double)n * Td);
        if (wrap != nullptr && wrap[r] != 0) m = wrap_pi(m);
        mean[r] = m;
        within[r] = var0;
        const double W = sw / halves, BL = sb / (halves - 1.0);
        rhat[r] = T >= 4u ? sqrt(((L - 1.0) / L * W + BL) / W) : (double)NAN;
        tau[r] = var0 / var0;                                          // 1, or NaN on a frozen row as at every level
    }
    for (int l = 1; l < levels; ++l) {
        const double* p = base + (size_t)(4 + 3 * (l - 1)) * plane;
        const double m = (double)(T >> l);
        double sl = 0.0;
        for (int i = tid; i < n; i += 256) {
            const double rs = p[plane + i], qs = p[2 * plane + i];
            sl += (qs - rs * rs / m) / (m - 1.0);
        }
        sl = block_sum(sl, part);
        if (tid == 0) tau[(size_t)l * (size_t)x_rows + (size_t)r] = (double)(1u << l) * (sl / (double)n) / var0;
    }
}

// x_rows, n >= 1, n <= 65535 * 64, 1 <= levels <= 16
inline bool shape(int x_rows, int n, int levels, unsigned* tiles) {
    if (x_rows < 1 || n < 1 || levels < 1 || levels > MAX_LEVELS) return false;
    const long long t = ((long long)n + TILE - 1) / TILE;
    if (t > 65535) return false;
    *tiles = (unsigned)t;
    return true;
}

// T even and >= 2, every level with at least two blocks: levels <= floor(log2 T)
inline bool length_ok(uint32_t T, int levels) { return T >= 2u && (T & 1u) == 0u && (T >> levels) >= 1u; }

}  // namespace

extern "C" size_t nfisam_chain_state_count(int x_rows, int n, int levels) {
    unsigned tiles;
    if (!shape(x_rows, n, levels, &tiles)) return 0;
    return (size_t)(4 + 3 * (levels - 1)) * (size_t)x_rows * (size_t)n;
}

extern "C" int nfisam_chain_record(const float* Xt, double* state, int x_rows, int n, int levels, const double* center,
                                   const uint8_t* wrap, uint32_t t, uint32_t T, nfisam_stream_t stream) {
    if (Xt == nullptr || state == nullptr) return NFISAM_ERR_ARG;
    unsigned tiles;
    if (!shape(x_rows, n, levels, &tiles) || !length_ok(T, levels) || t >= T) return NFISAM_ERR_ARG;
    const long long groups = ((long long)x_rows + 3) / 4;
    hipLaunchKernelGGL(chain_record_kernel, dim3(tiles, (unsigned)(groups < 65535 ? groups : 65535)), dim3(256), 0,
                       (hipStream_t)stream, Xt, state, x_rows, n, levels, center, wrap, t, t >= T / 2 ? 1 : 0);
    return launch_status(hipGetLastError());
}

extern "C" int nfisam_chain_finish(const double* state, int x_rows, int n, int levels, uint32_t T, const double* center,
                                   const uint8_t* wrap, double* mean, double* within, double* rhat, double* tau,
                                   nfisam_stream_t stream) {
    if (state == nullptr || mean == nullptr || within == nullptr || rhat == nullptr || tau == nullptr) return NFISAM_ERR_ARG;
    unsigned tiles;
    if (!shape(x_rows, n, levels, &tiles) || !length_ok(T, levels)) return NFISAM_ERR_ARG;
    hipLaunchKernelGGL(chain_finish_kernel, dim3((unsigned)x_rows), dim3(256), 0, (hipStream_t)stream, state, x_rows, n, levels, T,
                       center, wrap, mean, within, rhat, tau);
    return launch_status(hipGetLastError());
}
