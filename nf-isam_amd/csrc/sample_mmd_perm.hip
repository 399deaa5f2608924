// sample_mmd_perm.hip — the kernel sums of the two-sample MMD under many relabellings of the pooled set: the null
// distribution of the permutation test, every block of a table and every permutation of a call in one launch.
//
// Pooled set Z = [X; Y], N = m + n, K the block's kernel on Z (the formula, wrap and scale of sample_mmd.hip, word for word).
// A relabelling is l in {0,1}^N with m ones (1: "counts as the first set").  With t = K 1 and T = 1' K 1:
//     Sxx' = l' K l,    Sxy' = l' t - Sxx',    Syy' = T - 2 l' t + Sxx'.
// Every Gram value is evaluated once for 256 permutations and then costs one float64 multiply-add per permutation: the tile of
// kernel values is the A operand of v_mfma_f64_16x16x4_f64 and the labels, as 0.0 / 1.0, are the B operand.
//
// K is symmetric: only the upper triangle of the pooled tile grid is walked.  X is padded to a multiple of 64, so no tile
// straddles the two matrices and the pooled triangle is exactly sample_mmd.hip's three families (Sxx upper, Sxy full, Syy
// upper).  (1) a 256-thread group owns one tile ROW of that triangle (a strip: the diagonal tile first, then the tiles to its
// right), one block and one chunk of 256 permutations.  Per tile the four waves evaluate the 64 x 64 kernel values as
// sample_mmd.hip does (lane = i, 16 j a wave), park them in LDS, and then wave w multiplies the rows 16 w .. 16 w + 15 of the
// tile with the 64 x 256 label matrix of the tile's j: 16 k-steps x 16 column blocks, accumulated in 64 float64 registers a
// lane over the whole strip (the i of a strip never change).  The accumulators are folded twice a strip, after the diagonal
// tile and after the last one: masked by the i labels and plain, the four registers in order, the four lane groups by a fixed
// shuffle tree, the four waves in order.  With R_d / R_o the accumulators of the diagonal / the other tiles and r_i the row
// sums of the strip's kernel values the strip writes, per permutation,
//     q = sum_i l_i R_d,i + 2 sum_i l_i R_o,i        (its share of l' K l: the tiles right of the diagonal stand for two)
//     s = sum_i l_i r_i + sum_i R_o,i                (its share of l' t: rows i, and the columns j of the mirrored tiles)
// and once T_s = sum_i (r_d,i + 2 r_o,i): only sums of positive terms, P doubles per strip and kind, never per tile.
// (2) a thread per (block, permutation) adds the strips' q and s in strip order and writes {Sxx', Syy', Sxy'}.
//
// Numerics: float32 points in; differences, squared distance, exp, the MFMA and every sum float64 (sample_common.h).
// No float atomics; the order of every sum depends on (m, n) alone, and a permutation meets the others of its call only as
// other COLUMNS of an MFMA, which do not enter its own.  Hence: two calls give the same bits; a block's numbers are the same
// bits alone or anywhere in a table; a permutation's numbers are the same bits alone, first or last of a call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PCH = 256;          // permutations a group carries: 16 MFMA column blocks of 16
constexpr int PB = PCH / 16;      // column blocks
constexpr int PW = PCH / 64;      // label words per pooled point and chunk
static_assert(PCH == 256, "one thread per permutation of the chunk in the strip's epilogue");

// D = A B + C, A 16 x 4 (lane l: A[l & 15][l >> 4]), B 4 x 16 (lane l: B[l >> 4][l & 15]), D 16 x 16 (lane l, register r:
// D[(l >> 4) + 4 r][l & 15] -- NOT the row map of the float32 shapes)
__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// 1.0 where the bit is set, else 0.0
__device__ __forceinline__ double one_if(uint32_t bit) { return __hiloint2double((int)((0u - bit) & 0x3FF00000u), 0); }

template <bool WRAP, bool SCALE>
__device__ __forceinline__ void column_step(double (&acc)[JPL], double xi, const double* __restrict__ yrow, double sc) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        double diff = xi - yrow[jj];
        if (WRAP) diff = wrap_pi(diff);
        if (SCALE) diff *= sc;
        acc[jj] = fma(diff, diff, acc[jj]);
    }
}

// The accumulators of a wave's 16 rows folded over i, per permutation of the chunk: masked by the i labels and plain.  The
// four registers of a lane in order, the lane groups by a fixed tree, the waves in order; `red` is the (idle) tile buffer.
__device__ __forceinline__ void fold(const f64x4 (&C)[PB], const unsigned long long (*li)[PW], double* red, int w, int lane,
                                     double* masked, double* plain) {
    __syncthreads();                                               // every wave has read the tile
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int word = pb >> 2, sh = (pb & 3) * 16 + (lane & 15);
        double v = 0.0, u = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = 16 * w + (lane >> 4) + 4 * r;
            const double c = C[pb][r];
            v += ((li[il][word] >> sh) & 1ull) ? c : 0.0;
            u += c;
        }
        v += __shfl_down(v, 32, 64), u += __shfl_down(u, 32, 64);
        v += __shfl_down(v, 16, 64), u += __shfl_down(u, 16, 64);
        if (lane < 16) red[(0 * 4 + w) * PCH + pb * 16 + lane] = v, red[(1 * 4 + w) * PCH + pb * 16 + lane] = u;
    }
    __syncthreads();
    const int p = threadIdx.x;
    *masked = ((red[(0 * 4 + 0) * PCH + p] + red[(0 * 4 + 1) * PCH + p]) + red[(0 * 4 + 2) * PCH + p]) + red[(0 * 4 + 3) * PCH + p];
    *plain = ((red[(1 * 4 + 0) * PCH + p] + red[(1 * 4 + 1) * PCH + p]) + red[(1 * 4 + 2) * PCH + p]) + red[(1 * 4 + 3) * PCH + p];
    __syncthreads();                                               // the buffer is free for the next tile
}

// grid (strips of the pooled triangle, chunks of 256 permutations, blocks); 256 threads.  Two waves per SIMD: a second group
// evaluates its Gram tile while the first multiplies.  The 128 accumulator registers leave the Gram phase short of the 256
// that allows (59 spilled), and it still measured 14 % faster than one wave per SIMD without a spill.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) mmd_perm_strip_kernel(const nfisam_mmd_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                             int x_rows, int m, const float* __restrict__ Yt, int y_rows, int n,
                                                             const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                             int n_entries, const double* __restrict__ scale,
                                                             const uint8_t* __restrict__ wrap,
                                                             const unsigned long long* __restrict__ labels, int W, int Tx, int Tp,
                                                             int Ppad, double* __restrict__ part, double* __restrict__ tpart) {
    __shared__ double kt[TILE][TILE];                              // kt[j][i]; between tiles the buffer of `fold`
    __shared__ double ys[CH][TILE];
    __shared__ unsigned long long li[TILE][PW], lj[TILE][PW];      // the label words of the strip's i and of the tile's j
    __shared__ double rsw[2][4][TILE], rst[TILE];
    __shared__ int bad_any;
    static_assert(sizeof(double) * TILE * TILE >= sizeof(double) * 2 * 4 * PCH, "fold's buffer fits the tile");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int strip = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;

    // the i side: blockIdx alone decides, so all of it is wave-uniform
    const bool ix = strip < Tx;
    const float* __restrict__ A = ix ? Xt : Yt;
    const int32_t* __restrict__ acols = ix ? xcols : ycols;
    const int a_rows = ix ? x_rows : y_rows, an = ix ? m : n, qi0 = ix ? 0 : m, ti = ix ? strip : strip - Tx;

    const int col_off = blocks[b].col_off, d = blocks[b].d;
    const double inv = blocks[b].inv_two_sigma2;
    // a block whose entries leave the tables is never walked; a row outside its matrix is replaced by row 0: NaN either way
    bool bad = col_off < 0 || d < 1 || (long long)col_off + d > n_entries;
    const int d_walk = bad ? 0 : d;

    const int i = ti * TILE + lane;
    const size_t ic = (size_t)(i < an ? i : an - 1);
    if (tid == 0) bad_any = 0;
    {
        const int r = tid >> 2, k = tid & 3, ir = ti * TILE + r, gw = chunk * PW + k;      // 64 rows x 4 words: one a thread
        li[r][k] = (ir < an && gw < W) ? labels[(size_t)(qi0 + ir) * (size_t)W + (size_t)gw] : 0ull;
    }

    f64x4 C[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) C[pb] = f64x4{0.0, 0.0, 0.0, 0.0};
    double rd = 0.0, ro = 0.0;                                     // this wave's 16 j of the row sums of i: diagonal tile, others
    double q_diag = 0.0, unused = 0.0;

    for (int tjp = strip; tjp < Tp; ++tjp) {
        const bool jx = tjp < Tx;
        const float* __restrict__ B = jx ? Xt : Yt;
        const int32_t* __restrict__ bcols = jx ? xcols : ycols;
        const int b_rows = jx ? x_rows : y_rows, bn = jx ? m : n, qj0 = jx ? 0 : m, tj = jx ? tjp : tjp - Tx;
        const int jl = tj * TILE + lane;                           // the j this thread stages
        const size_t jc = (size_t)(jl < bn ? jl : bn - 1);

        __syncthreads();                                           // the previous tile and its labels have been read
        {
            const int r = tid >> 2, k = tid & 3, jr = tj * TILE + r, gw = chunk * PW + k;
            lj[r][k] = (jr < bn && gw < W) ? labels[(size_t)(qj0 + jr) * (size_t)W + (size_t)gw] : 0ull;
        }

        double acc[JPL];
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) acc[jj] = 0.0;

        for (int c0 = 0; c0 < d_walk; c0 += CH) {
            const int cnt = min(CH, d_walk - c0);
            if (c0 > 0) __syncthreads();                           // the previous chunk's columns have been read
#pragma unroll
            for (int k = 0; k < CH / 4; ++k) {                     // wave w stages columns w, w + 4, ...
                const int c = w + 4 * k;
                if (c < cnt) {
                    int row = bcols[col_off + c0 + c];
                    if (row < 0 || row >= b_rows) bad = true, row = 0;
                    ys[c][lane] = (double)B[(size_t)row * bn + jc];
                }
            }
            float xa[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {                         // the i side: one coalesced row read per column
                xa[c] = 0.0f;
                if (c < cnt) {
                    int row = acols[col_off + c0 + c];
                    if (row < 0 || row >= a_rows) bad = true, row = 0;
                    xa[c] = A[(size_t)row * an + ic];
                }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (c < cnt) {
                    const int e = col_off + c0 + c;
                    const bool wr = wrap != nullptr && wrap[e] != 0;
                    const double xi = (double)xa[c];
                    const double* __restrict__ yrow = &ys[c][w * JPL];
                    if (scale != nullptr) {
                        const double sc = scale[e];
                        if (wr) column_step<true, true>(acc, xi, yrow, sc);
                        else column_step<false, true>(acc, xi, yrow, sc);
                    } else {
                        if (wr) column_step<true, false>(acc, xi, yrow, 1.0);
                        else column_step<false, false>(acc, xi, yrow, 1.0);
                    }
                }
            }
        }

        double s = 0.0;
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) {
            const int j = tj * TILE + w * JPL + jj;
            const double k = (i < an && j < bn) ? exp(-inv * acc[jj]) : 0.0;
            kt[w * JPL + jj][lane] = k;
            s += k;
        }
        if (tjp == strip) rd += s;
        else ro += s;
        __syncthreads();

        // rows 16 w .. 16 w + 15 of the tile times the labels of its 64 j: lane l brings A[i = l & 15][j = 4 ks + (l >> 4)] and,
        // per column block, B[j][p = l & 15]
        {
            const int il = 16 * w + (lane & 15), kq = lane >> 4, sh = lane & 15;
#pragma unroll 2
            for (int ks = 0; ks < TILE / 4; ++ks) {
                const int j = 4 * ks + kq;
                const double a = kt[j][il];
#pragma unroll
                for (int k = 0; k < PW; ++k) {
                    const unsigned long long t = lj[j][k] >> sh;
                    const uint32_t lo = (uint32_t)t, hi = (uint32_t)(t >> 32);
                    C[4 * k + 0] = mfma_f64(a, one_if(lo & 1u), C[4 * k + 0]);
                    C[4 * k + 1] = mfma_f64(a, one_if((lo >> 16) & 1u), C[4 * k + 1]);
                    C[4 * k + 2] = mfma_f64(a, one_if(hi & 1u), C[4 * k + 2]);
                    C[4 * k + 3] = mfma_f64(a, one_if((hi >> 16) & 1u), C[4 * k + 3]);
                }
            }
        }

        if (tjp == strip) {                                        // the diagonal tile stands for itself, the others for two
            fold(C, li, &kt[0][0], w, lane, &q_diag, &unused);
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) C[pb] = f64x4{0.0, 0.0, 0.0, 0.0};
        }
    }

    double q_off, col_off_sum;
    fold(C, li, &kt[0][0], w, lane, &q_off, &col_off_sum);

    // the row sums of the strip: the four waves' shares in order; `bad` is uniform within a wave but each wave has seen only
    // the rows it staged
    rsw[0][w][lane] = rd, rsw[1][w][lane] = ro;
    if (bad) bad_any = 1;
    __syncthreads();
    if (tid < TILE) {
        const double rdt = ((rsw[0][0][tid] + rsw[0][1][tid]) + rsw[0][2][tid]) + rsw[0][3][tid];
        const double rot = ((rsw[1][0][tid] + rsw[1][1][tid]) + rsw[1][2][tid]) + rsw[1][3][tid];
        rst[tid] = rdt + rot;
        const double tsum = wave_sum(rdt + 2.0 * rot);
        if (tid == 0 && chunk == 0) tpart[(size_t)b * (size_t)Tp + (size_t)strip] = bad_any ? (double)NAN : tsum;
    }
    __syncthreads();
    double lr = 0.0;                                               // sum_i l_i r_i of permutation tid, i ascending
    {
        const int word = tid >> 6, sh = tid & 63;
        for (int r = 0; r < TILE; ++r) lr += ((li[r][word] >> sh) & 1ull) ? rst[r] : 0.0;
    }
    const bool any = bad_any != 0;
    double* __restrict__ out = part + ((size_t)b * (size_t)Tp + (size_t)strip) * 2 * (size_t)Ppad + (size_t)chunk * PCH + tid;
    out[0] = any ? (double)NAN : q_diag + 2.0 * q_off;
    out[Ppad] = any ? (double)NAN : lr + col_off_sum;
}

// grid (chunks of 256 permutations, blocks): a thread per permutation adds the strips in order -- an order that depends on
// (m, n) alone
__global__ void __launch_bounds__(256) mmd_perm_finish_kernel(const double* __restrict__ part, const double* __restrict__ tpart,
                                                              int Tp, int Ppad, int n_perms, double* __restrict__ sums) {
    const int p = blockIdx.x * PCH + threadIdx.x, b = blockIdx.y;
    if (p >= n_perms) return;
    double q = 0.0, s = 0.0, T = 0.0;
    for (int k = 0; k < Tp; ++k) {
        const double* __restrict__ in = part + ((size_t)b * (size_t)Tp + (size_t)k) * 2 * (size_t)Ppad + (size_t)p;
        q += in[0];
        s += in[Ppad];
        T += tpart[(size_t)b * (size_t)Tp + (size_t)k];
    }
    double* __restrict__ o = sums + ((size_t)b * (size_t)n_perms + (size_t)p) * 3;
    o[0] = q;
    o[1] = (T - 2.0 * s) + q;
    o[2] = s - q;
}

// the pooled tile grid and the permutation chunks, if the launch can hold them
bool shape(int m, int n, int n_blocks, int n_perms, int* Tx, int* Tp, int* chunks) {
    int Ty;
    if (n_blocks < 1 || n_blocks > 65535 || n_perms < 1 || n_perms > NFISAM_MMD_PERM_MAX) return false;
    if (!tile_count(m, Tx) || !tile_count(n, &Ty)) return false;
    *Tp = *Tx + Ty;
    *chunks = (n_perms + PCH - 1) / PCH;
    return (long long)*Tp * *chunks * n_blocks <= 16777215LL;     // 256 threads a group: 2^32 threads at the most
}

}  // namespace

extern "C" size_t nfisam_sample_mmd_perm_scratch_count(int m, int n, int n_blocks, int n_perms) {
    int Tx, Tp, chunks;
    if (!shape(m, n, n_blocks, n_perms, &Tx, &Tp, &chunks)) return 0;
    return (size_t)n_blocks * (size_t)Tp * (2 * (size_t)chunks * PCH + 1);   // q and s per (block, strip, permutation), T per strip
}

extern "C" int nfisam_sample_mmd_perm(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n,
                                      const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev, int n_blocks,
                                      const int32_t* xcols, const int32_t* ycols, int n_entries, const double* scale,
                                      const uint8_t* wrap, const uint64_t* labels, int n_perms, double* sums, double* scratch,
                                      nfisam_stream_t stream) {
    if (Xt == nullptr || Yt == nullptr || blocks == nullptr || blocks_dev == nullptr || xcols == nullptr || ycols == nullptr ||
        labels == nullptr || sums == nullptr || scratch == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || y_rows < 1 || n_entries < 1) return NFISAM_ERR_ARG;
    int Tx, Tp, chunks;
    if (!shape(m, n, n_blocks, n_perms, &Tx, &Tp, &chunks)) return NFISAM_ERR_ARG;
    if (!check_block_table(blocks, n_blocks)) return NFISAM_ERR_ARG;   // `blocks` is the HOST copy of the table
    hipStream_t s = (hipStream_t)stream;
    const int Ppad = chunks * PCH, W = (n_perms + 63) / 64;
    double* part = scratch;
    double* tpart = scratch + (size_t)n_blocks * (size_t)Tp * 2 * (size_t)Ppad;
    hipLaunchKernelGGL(mmd_perm_strip_kernel, dim3(Tp, chunks, n_blocks), dim3(256), 0, s, blocks_dev, Xt, x_rows, m, Yt, y_rows, n,
                       xcols, ycols, n_entries, scale, wrap, (const unsigned long long*)labels, W, Tx, Tp, Ppad, part, tpart);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mmd_perm_finish_kernel, dim3(chunks, n_blocks), dim3(256), 0, s, part, tpart, Tp, Ppad, n_perms, sums);
        e = hipGetLastError();
    }
    return launch_status(e);
}
