// fv_fit.h -- the fit layer's device code and launchers: the row passes of the fused objective and of the Gauss-Newton
// product (without calibration, with per-antenna gains, with 2 x 2 Jones matrices), their gradient gathers, and the
// kernels of the two alternating solves.  Needs fv_common.h alone; fv_sim.h (the handle's calls) and fv_capi.hip (the
// stand-alone calls) launch what stands here.
#pragma once

#include "fv_common.h"

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <type_traits>

namespace fv {

// ---------------------------------------------------------------------------------------------
// Row passes of a fit (DESIGN.md "Fused objective": the row walk).  A block of visibilities is nrows = nf nt rows of
// L = tpol nbls contiguous complex values.  k_residual_rows (the objective) and k_weight_rows (the Gauss-Newton product)
// walk it the same way, with and without per-antenna gains, and differ in their element function alone.  The pieces of
// the walk stand here, once:
//   Chunks (row_chunk, ChunkC, ChunkW).  One thread <-> one chunk of RES_W<T> = 16 / sizeof(T) elements aligned in the
// BLOCK's own index (not the row's): 16 bytes of weights and twice 16 bytes of every complex array, read and written as
// 16-byte vectors when all the arrays are 16-byte aligned (vec) and the chunk lies inside the row; the first and the last
// chunk of a row are clipped to it and go element by element.  A block takes RES_CHUNKS consecutive groups of 256 chunks
// of its row; the grid is (blocks per row, rows), and rows beyond the grid's y limit are walked with its stride.
//   Row term (row_term).  What an element adds to its row's sum, w |x|^2, is formed in fp64 with one fused multiply-add,
// the real part's square the fused one, written out so that every kernel, instance and path rounds it alike.
//   Row tail (row_tail).  Every block writes ONE fp64 partial, partials[row][block]: per thread in chunk order, an
// __shfl_xor tree inside the wave, then the waves in order through LDS.  k_chi2_rows_reduce adds a row's partials in
// index order.  No floating-point atomics: the sums' bits depend on the input alone.  Bad input is counted on the way
// (int atomics): bad[0] weights that are negative or not finite, bad[1] data that are not finite where w > 0.
//   Gain view (GainView; the gains' layout and the feeds: "Per-antenna gains" below).  Element e of a row has
// pol = e / nbls, k = e % nbls: a chunk finds (pol, k) of its first element with one division and carries them.  The
// row's gains -- and their direction, when both fit GAIN_LDS_BYTES together -- are staged in dynamic LDS.  With
// GAINS = false every member function is empty: no division, no index loads, no dynamic LDS.
template <typename T>
constexpr int RES_W = 16 / (int)sizeof(T);
constexpr int RES_CHUNKS = 4;
constexpr size_t GAIN_LDS_BYTES = 32768;
struct RowChunk {
    int64_t e0, a, b;  // the chunk's first element in the block's index, and its part [a, b) inside the row
    bool whole;        // all of it inside the row, and vectors allowed
};
// chunk i (< RES_CHUNKS) of this thread in the row [lo, hi) of the block's index, c0 = lo / RES_W<T> the row's first
// chunk; e0 >= hi: at or past the row's end, and so are the thread's later chunks.  (By value, with c0 from the kernel:
// filling a reference and returning "ended" cost k_residual_rows<double, true> two VGPRs and with them occupancy 8.)
template <typename T>
__device__ __forceinline__ RowChunk row_chunk(int64_t c0, int64_t lo, int64_t hi, int i, int vec) {
    constexpr int W = RES_W<T>;
    const int64_t e0 = (c0 + ((int64_t)blockIdx.x * RES_CHUNKS + i) * 256 + threadIdx.x) * W;
    return {e0, e0 > lo ? e0 : lo, e0 + W < hi ? e0 + W : hi, vec && e0 >= lo && e0 + W <= hi};
}
template <typename T>
union ChunkC {  // a whole chunk of complex values: two 16-byte vectors
    static constexpr int NV = RES_W<T> * (int)sizeof(cplx<T>) / 16;
    uint4 q[NV];
    cplx<T> c[RES_W<T>];
    __device__ __forceinline__ void load(const cplx<T> *p) {
#pragma unroll
        for (int k = 0; k < NV; ++k) q[k] = reinterpret_cast<const uint4 *>(p)[k];
    }
    __device__ __forceinline__ void store(cplx<T> *p) const {
#pragma unroll
        for (int k = 0; k < NV; ++k) reinterpret_cast<uint4 *>(p)[k] = q[k];
    }
};
template <typename T>
union ChunkW {  // a whole chunk of weights: one 16-byte vector
    uint4 q;
    T w[RES_W<T>];
    __device__ __forceinline__ void load(const T *p) { q = *reinterpret_cast<const uint4 *>(p); }
};
template <typename T>
__device__ __forceinline__ double row_term(T w, T xr, T xi) {
#pragma clang fp contract(off)
    const double dr = (double)xr, di = (double)xi;
    return (double)w * __builtin_fma(dr, dr, di * di);
}
// a thread's sum s and its counts of bad input -> the block's partial of `row` and the counters; the closing barrier
// lets the next row of this block write wave_sum, and the staged gains, again
__device__ __forceinline__ void row_tail(double s, int bad_w, int bad_d, int64_t row, double *__restrict__ partials,
                                         int *__restrict__ bad) {
    __shared__ double wave_sum[4];
    if (bad_w) atomicAdd(bad, bad_w);
    if (bad_d) atomicAdd(bad + 1, bad_d);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[row * gridDim.x + blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
    __syncthreads();
}
__device__ __forceinline__ void gain_feeds(int pol, int nfeed, int &p, int &q) {  // p: a1's feed, q: a2's
    p = nfeed == 2 ? (pol & 1) : 0;
    q = nfeed == 2 ? (pol >> 1) : 0;
}
template <typename T>
struct PairGains {  // of one element: g1 = g[p, a1], g2 = g[q, a2], and the direction's h1, h2 (0 without one)
    cplx<T> g1, g2, h1, h2;
};
template <typename T, bool GAINS>
struct GainView {
    const cplx<T> *gains, *dgains;  // the block's (nrows, nfeed nant); dgains null: no direction
    const int *ant1, *ant2;
    int nbls, nant, nfeed, in_lds;
    const cplx<T> *g, *h;  // the row's, after stage()
    int pol, k, p, q;      // of the current element, after seek()
    __device__ __forceinline__ void stage(int64_t row) {
        if constexpr (GAINS) {
            extern __shared__ __align__(16) unsigned char gain_lds[];
            const int ng = nfeed * nant;
            g = gains + row * ng;
            h = dgains ? dgains + row * ng : nullptr;
            if (in_lds) {
                cplx<T> *gl = reinterpret_cast<cplx<T> *>(gain_lds);
                for (int i = threadIdx.x; i < ng; i += 256) gl[i] = g[i];
                g = gl;
                if (h) {
                    for (int i = threadIdx.x; i < ng; i += 256) gl[ng + i] = h[i];
                    h = gl + ng;
                }
                __syncthreads();
            }
        }
    }
    __device__ __forceinline__ void seek(int64_t e) {  // to element e of the row
        if constexpr (GAINS) {
            pol = (int)(e / nbls);
            k = (int)(e - (int64_t)pol * nbls);
            gain_feeds(pol, nfeed, p, q);
        }
    }
    __device__ __forceinline__ void next() {
        if constexpr (GAINS) {
            if (++k == nbls) {
                k = 0;
                gain_feeds(++pol, nfeed, p, q);
            }
        }
    }
    __device__ __forceinline__ PairGains<T> pair() const {
        const cplx<T> zero = {(T)0, (T)0};
        if constexpr (GAINS) {
            const int i1 = p * nant + ant1[k], i2 = q * nant + ant2[k];
            return {g[i1], g[i2], h ? h[i1] : zero, h ? h[i2] : zero};
        }
        return {zero, zero, zero, zero};
    }
};

// ---------------------------------------------------------------------------------------------
// Fused objective (fv_residual_chi2, fv_sim_run_residual) and per-antenna gains in it (fv_gain_residual_chi2,
// fv_sim_run_residual_gains); DESIGN.md "Fused objective", "Gains".  In place, per element of the block V,
//     delta = V - d (T),   G = 2 w delta (T: two roundings and an exact doubling),   row sum += w |delta|^2 (row_term),
// w = 1 without weights.  w == 0 flags the sample: G = 0 exactly, nothing is added and d is not used (a select, so NaN or
// Inf there do not propagate).  With gains (GAINS; g1, g2 of the element's baseline: "Per-antenna gains" below)
//     m = conj(g1) g2,   V' = m V,   delta = V' - d,   G' = 2 (w delta),   stored G = conj(m) G',   row sum += w |delta|^2.
// In T every operation rounds on its own (no contraction): the same arithmetic on any compiler, reproducible operation
// by operation in a test.  The products are written out: the pragma is lexical and would not reach cmul.  With unit
// gains m = 1 and the two instances give the same bits.
template <typename T, bool GAINS>
__device__ __forceinline__ double residual_element(cplx<T> &v, const cplx<T> &d, T w, const PairGains<T> &pg, int &bad_w,
                                                   int &bad_d) {
#pragma clang fp contract(off)
    if (!(w >= (T)0) || !isfinite(w)) ++bad_w;
    if (!(w > (T)0)) {  // flagged (or counted above)
        v = {(T)0, (T)0};
        return 0.0;
    }
    if (!isfinite(d.re) || !isfinite(d.im)) ++bad_d;
    T dr, di;
    if constexpr (GAINS) {
        const cplx<T> &g1 = pg.g1, &g2 = pg.g2;
        const T mr = g1.re * g2.re + g1.im * g2.im, mi = g1.re * g2.im - g1.im * g2.re;  // m = conj(g1) g2
        dr = (mr * v.re - mi * v.im) - d.re;                                             // delta = m V - d
        di = (mr * v.im + mi * v.re) - d.im;
        const T gr = (T)2 * (w * dr), gi = (T)2 * (w * di);  // G'
        v = {mr * gr + mi * gi, mr * gi - mi * gr};          // conj(m) G'
    } else {
        dr = v.re - d.re;
        di = v.im - d.im;
        v = {(T)2 * (w * dr), (T)2 * (w * di)};
    }
    return row_term<T>(w, dr, di);
}
template <typename T, bool GAINS>
__global__ void __launch_bounds__(256)
    k_residual_rows(cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                    const cplx<T> *__restrict__ gains, const int *__restrict__ ant1, const int *__restrict__ ant2, int64_t nrows,
                    int64_t L, int nbls, int nant, int nfeed, int in_lds, int vec, double *__restrict__ partials,
                    int *__restrict__ bad) {
    constexpr int W = RES_W<T>;
    GainView<T, GAINS> gv{gains, nullptr, ant1, ant2, nbls, nant, nfeed, in_lds};
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        gv.stage(row);
        const int64_t lo = row * L, hi = lo + L, c0 = lo / W;  // the row in the block's index, and its first chunk
        double s = 0.0;
        int bad_w = 0, bad_d = 0;
        for (int i = 0; i < RES_CHUNKS; ++i) {
            const RowChunk c = row_chunk<T>(c0, lo, hi, i, vec);
            if (c.e0 >= hi) break;
            gv.seek(c.a - lo);
            if (c.whole) {
                ChunkC<T> v, d;
                ChunkW<T> ww;
                v.load(vis + c.e0);
                d.load(data + c.e0);
                if (weights) ww.load(weights + c.e0);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    s += residual_element<T, GAINS>(v.c[j], d.c[j], weights ? ww.w[j] : (T)1, gv.pair(), bad_w, bad_d);
                    gv.next();
                }
                v.store(vis + c.e0);
            } else {
                for (int64_t e = c.a; e < c.b; ++e) {
                    cplx<T> v = vis[e];
                    s += residual_element<T, GAINS>(v, data[e], weights ? weights[e] : (T)1, gv.pair(), bad_w, bad_d);
                    vis[e] = v;
                    gv.next();
                }
            }
        }
        row_tail(s, bad_w, bad_d, row, partials, bad);
    }
}
// chi2_rows[row] = a row's partials added in index order (row_tail)
__global__ void k_chi2_rows_reduce(const double *__restrict__ partials, int64_t nrows, int nblk, double *__restrict__ chi2_rows) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partials[row * nblk + b];
    chi2_rows[row] = s;
}
// blocks per row of a row pass: the chunks a row of L elements can touch (one more than its own when it starts inside a
// chunk), RES_CHUNKS * 256 per block
template <typename T>
inline int residual_blocks_per_row(int64_t L) {
    return (int)std::max<int64_t>(1, cdiv(cdiv(L, RES_W<T>) + 1, (int64_t)RES_CHUNKS * 256));
}
// A row pass's scratch, carved out of one buffer (reserved here): partials nrows * nblk doubles, the rows' sums nrows
// doubles, then the two counters.
struct RowScratch {
    int nblk;  // blocks per row
    double *partials, *sums;
    int *bad;
};
template <typename T>
inline RowScratch row_scratch(DevBuf &buf, int64_t nrows, int64_t L) {
    const int nblk = residual_blocks_per_row<T>(L);
    buf.reserve(sizeof(double) * (size_t)nrows * (nblk + 1) + 16);
    double *partials = buf.as<double>(), *sums = partials + (size_t)nrows * nblk;
    return {nblk, partials, sums, reinterpret_cast<int *>(sums + nrows)};
}
// the message of a call that met bad input (row_tail's counters)
inline void throw_if_bad_residual_input(const int bad[2]) {
    if (bad[0])
        throw Error(FV_ERR_ARG, std::to_string(bad[0]) + " weights are negative or not finite (weights are inverse variances; 0 "
                                                         "flags a sample)");
    if (bad[1])
        throw Error(FV_ERR_ARG, std::to_string(bad[1]) + " entries of data are not finite where the weight is positive (flag "
                                                         "them with weight 0)");
}
// What every row pass ends with: the rows' sums and the counters come to the host (hbad) behind whatever else the caller
// queued on `on`, with one synchronisation.
inline void collect_rows(hipStream_t on, const RowScratch &rs, int64_t nrows, double *rows_host, int hbad[2]) {
    hbad[0] = hbad[1] = 0;
    FV_HIP(hipMemcpyAsync(rows_host, rs.sums, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, on));
    FV_HIP(hipMemcpyAsync(hbad, rs.bad, 2 * sizeof(int), hipMemcpyDeviceToHost, on));
    FV_HIP(hipStreamSynchronize(on));
    FV_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// Gauss-Newton product (fv_weight_rows, fv_sim_weight_block) and the same with per-antenna gains and a gain direction
// (fv_gain_weight_rows, fv_sim_gain_weight_block); DESIGN.md "Gauss-Newton product", "Gains in the Gauss-Newton product".
// The tangent J p of a block arrives as NP part blocks P_0 .. P_{NP-1} of the block's shape (one per tangent pass); per
// element, in the run's precision T and in this order,
//     U = ((P_0 + P_1) + P_2) + P_3 (component-wise, only the parts given),   G = 2 (w U) (one rounding per component
//     and an exact doubling),   row sum += w |U|^2 (row_term),
// w = 1 without weights; G replaces P_0.  w == 0 flags the sample: G = 0 exactly, nothing is added and the parts are not
// used there (a select).  NP = 1 .. 4.  With gains (GAINS; NP = 0 .. 4, U = 0 for NP = 0, the gains-only direction), V the
// forward at the real parameters and h1, h2 the direction's entries where the gains have g1, g2,
//     m = conj(g1) g2,   dm = conj(h1) g2 + conj(g1) h2 (dm = 0 without a gain direction),   U' = m U + dm V,
//     G' = 2 (w U'),   stored G = conj(m) G',   row sum += w |U'|^2.
// V is read only with a gain direction; G replaces P_0, or V for NP = 0.  In T every operation rounds on its own, in the
// order written (residual_element): with unit gains and no direction m = 1, m U = U and conj(m) G' = G' exactly, and the
// two instances give the same bits.  bad[0] counts the weights that are negative or not finite, bad[1] stays 0.
template <typename T>
struct WeightParts {
    cplx<T> *p[4];
};
template <typename T, bool GAINS>
__device__ __forceinline__ double weight_element(cplx<T> &u, const cplx<T> &v, T w, const PairGains<T> &pg, bool sky, bool dir,
                                                 int &bad_w) {
#pragma clang fp contract(off)
    if (!(w >= (T)0) || !isfinite(w)) ++bad_w;
    if (!(w > (T)0)) {  // flagged (or counted above)
        u = {(T)0, (T)0};
        return 0.0;
    }
    T ur = u.re, ui = u.im;
    if constexpr (GAINS) {
        const cplx<T> &g1 = pg.g1, &g2 = pg.g2, &h1 = pg.h1, &h2 = pg.h2;
        const T mr = g1.re * g2.re + g1.im * g2.im, mi = g1.re * g2.im - g1.im * g2.re;  // m = conj(g1) g2
        ur = mr * u.re - mi * u.im;                                                      // m U
        ui = mr * u.im + mi * u.re;
        if (dir) {
            const T dmr = (h1.re * g2.re + h1.im * g2.im) + (g1.re * h2.re + g1.im * h2.im);  // dm = conj(h1) g2 + conj(g1) h2
            const T dmi = (h1.re * g2.im - h1.im * g2.re) + (g1.re * h2.im - g1.im * h2.re);
            const T tr = dmr * v.re - dmi * v.im, ti = dmr * v.im + dmi * v.re;  // dm V
            ur = sky ? ur + tr : tr;                                             // U' = m U + dm V (dm V alone for NP = 0)
            ui = sky ? ui + ti : ti;
        }
        const T gr = (T)2 * (w * ur), gi = (T)2 * (w * ui);  // G'
        u = {mr * gr + mi * gi, mr * gi - mi * gr};          // conj(m) G'
    } else {
        u = {(T)2 * (w * ur), (T)2 * (w * ui)};
    }
    return row_term<T>(w, ur, ui);
}
template <typename T, int NP, bool GAINS>
__global__ void __launch_bounds__(256)
    k_weight_rows(WeightParts<T> parts, cplx<T> *__restrict__ vis, const T *__restrict__ weights, const cplx<T> *__restrict__ gains,
                  const cplx<T> *__restrict__ dgains, const int *__restrict__ ant1, const int *__restrict__ ant2, int64_t nrows,
                  int64_t L, int nbls, int nant, int nfeed, int in_lds, int vec, double *__restrict__ partials,
                  int *__restrict__ bad) {
    static_assert(NP >= (GAINS ? 0 : 1) && NP <= 4, "NP = 1 .. 4, or 0 .. 4 with gains");
    constexpr int W = RES_W<T>;
    GainView<T, GAINS> gv{gains, dgains, ant1, ant2, nbls, nant, nfeed, in_lds};
    const bool dir = GAINS && dgains != nullptr;
    cplx<T> *const out = NP ? parts.p[0] : vis;  // where G goes
    const cplx<T> zero = {(T)0, (T)0};
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        gv.stage(row);
        const int64_t lo = row * L, hi = lo + L, c0 = lo / W;  // the row in the block's index, and its first chunk
        double s = 0.0;
        int bad_w = 0;
        for (int i = 0; i < RES_CHUNKS; ++i) {
            const RowChunk c = row_chunk<T>(c0, lo, hi, i, vec);
            if (c.e0 >= hi) break;
            gv.seek(c.a - lo);
            if (c.whole) {
                ChunkC<T> u, t;
                ChunkW<T> ww;
                if (NP) {
                    u.load(parts.p[0] + c.e0);
#pragma unroll
                    for (int n = 1; n < NP; ++n) {
                        t.load(parts.p[n] + c.e0);
#pragma unroll
                        for (int j = 0; j < W; ++j) u.c[j] = {u.c[j].re + t.c[j].re, u.c[j].im + t.c[j].im};
                    }
                }
                if (dir) t.load(vis + c.e0);
                if (weights) ww.load(weights + c.e0);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    if (!NP) u.c[j] = zero;
                    s += weight_element<T, GAINS>(u.c[j], dir ? t.c[j] : zero, weights ? ww.w[j] : (T)1, gv.pair(), NP != 0, dir,
                                                  bad_w);
                    gv.next();
                }
                u.store(out + c.e0);
            } else {
                for (int64_t e = c.a; e < c.b; ++e) {
                    cplx<T> u = zero;
                    if (NP) u = parts.p[0][e];
#pragma unroll
                    for (int n = 1; n < NP; ++n) u = {u.re + parts.p[n][e].re, u.im + parts.p[n][e].im};
                    s += weight_element<T, GAINS>(u, dir ? vis[e] : zero, weights ? weights[e] : (T)1, gv.pair(), NP != 0, dir,
                                                  bad_w);
                    out[e] = u;
                    gv.next();
                }
            }
        }
        row_tail(s, bad_w, 0, row, partials, bad);
    }
}

// ---------------------------------------------------------------------------------------------
// Per-antenna gains (fv_gain_residual_chi2, fv_sim_run_residual_gains; DESIGN.md "Gains").  The block is the row
// passes': nrows rows of L = tpol nbls values, element e of a row has pol = e / nbls, k = e % nbls.
// Baseline k = (a1, a2) = (ant1[k], ant2[k]); a row's gains are nfeed nant complex values of the run's precision,
// g[feed nant + ant], nfeed = 1 (tpol 1) or 2 (tpol 4).  Of the polarized output's two feed axes the MINOR one is
// antenna a1's (the conjugated one; out[.., x, y, k] = (A_a1^H C A_a2)[y, x]): pol = 2 q + p with p a1's feed and q a2's.
// With m, V', delta and G' of k_residual_rows<T, true>,
//     ggains[a, f] = sum_{k: a1 = a, p = f} conj(G') g[a2, q] V + sum_{k: a2 = a, q = f} G' g[a1, p] conj(V).
// Two kernels, no floating-point atomics.  k_gain_gradient runs first, while the block still holds V: a gather over the
// per-antenna incidence lists (CSR; entry = 2 k + side, ascending, side 0 = "a is a1"), one wave per (row, feed, antenna),
// lane l takes the entries l, l + 64, ... in order, everything in fp64 from the T-typed inputs, an __shfl_xor tree, one
// complex128 per wave.  k_residual_rows<T, true> follows.
// ggains[(row nfeed + feed) nant + a]: one wave per (row, feed, antenna); see above.  vis still holds V.
template <typename T>
__global__ void __launch_bounds__(256)
    k_gain_gradient(const cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                    const cplx<T> *__restrict__ gains, const int *__restrict__ ant1, const int *__restrict__ ant2,
                    const int *__restrict__ inc_off, const int *__restrict__ inc, int64_t nrows, int nbls, int tpol, int nant,
                    cplx<double> *__restrict__ ggains) {
    const int nfeed = tpol == 4 ? 2 : 1, ng = nfeed * nant;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (wave >= ng) return;  // (whole waves: the tree below stays inside one)
    const int feed = wave / nant, ant = wave - feed * nant;
    const int i0 = inc_off[ant], i1 = inc_off[ant + 1];
    const int64_t L = (int64_t)tpol * nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *g = gains + row * ng;
        double sr = 0.0, si = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            for (int o = 0; o < nfeed; ++o) {  // the other antenna's feed
                const int p = side ? o : feed, q = side ? feed : o;
                const int64_t e = row * L + (int64_t)(nfeed == 2 ? 2 * q + p : 0) * nbls + k;
                const T wt = weights ? weights[e] : (T)1;
                if (!(wt > (T)0)) continue;  // flagged: nothing is added, the datum is not read
                const cplx<double> g1 = {(double)g[p * nant + a1].re, (double)g[p * nant + a1].im};
                const cplx<double> g2 = {(double)g[q * nant + a2].re, (double)g[q * nant + a2].im};
                const cplx<double> v = {(double)vis[e].re, (double)vis[e].im};
                const cplx<double> vp = cmul(cmul(cconj(g1), g2), v);
                const double w2 = 2.0 * (double)wt;
                const cplx<double> gp = {w2 * (vp.re - (double)data[e].re), w2 * (vp.im - (double)data[e].im)};
                // side 0: conj(G') g2 V;  side 1: G' g1 conj(V)
                const cplx<double> t = side ? cmul(gp, cmul(g1, cconj(v))) : cmul(cconj(gp), cmul(g2, v));
                sr += t.re;
                si += t.im;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off, 64);
            si += __shfl_xor(si, off, 64);
        }
        if (lane == 0) ggains[(row * nfeed + feed) * nant + ant] = {sr, si};
    }
}
// The per-antenna incidence lists of the pairs (ant1[k], ant2[k]), k < nbls: off[a] .. off[a + 1] are antenna a's entries
// 2 k + side in ascending order (side 0: a is ant1[k]; an auto-correlation has both).  An index outside [0, nant) is
// FV_ERR_ARG.
inline void gain_incidence(int nant, int64_t nbls, const int *ant1, const int *ant2, std::vector<int> &off, std::vector<int> &inc) {
    FV_REQUIRE(nant >= 1 && nbls >= 0 && nbls < ((int64_t)1 << 30) && (nbls == 0 || (ant1 && ant2)), "gain pairs: bad nant, nbls or null pairs");
    for (int64_t k = 0; k < nbls; ++k)
        FV_REQUIRE(ant1[k] >= 0 && ant1[k] < nant && ant2[k] >= 0 && ant2[k] < nant, "gain pairs: antenna index outside [0, nant)");
    off.assign((size_t)nant + 1, 0);
    for (int64_t k = 0; k < nbls; ++k) {
        ++off[ant1[k] + 1];
        ++off[ant2[k] + 1];
    }
    for (int a = 0; a < nant; ++a) off[a + 1] += off[a];
    inc.assign((size_t)2 * nbls, 0);
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int64_t k = 0; k < nbls; ++k) {
        inc[at[ant1[k]]++] = (int)(2 * k);
        inc[at[ant2[k]]++] = (int)(2 * k + 1);
    }
}
// The pairs and their incidence lists on the device (one set per handle, or per fv_gain_residual_chi2 call)
struct GainPairs {
    DevBuf d_ant1, d_ant2, d_off, d_inc;
    int nant = 0;
    int64_t nbls = -1;  // -1: not set
    std::vector<int> h_ant1, h_ant2;  // what the device holds while nbls >= 0: the same pairs again cost two compares
    void set(hipStream_t on, int nant_, int64_t nbls_, const int *ant1, const int *ant2) {
        if (nbls >= 0 && nbls_ == nbls && nant_ == nant && (nbls_ == 0 || (ant1 && ant2)) &&
            std::equal(h_ant1.begin(), h_ant1.end(), ant1) && std::equal(h_ant2.begin(), h_ant2.end(), ant2))
            return;  // (a solver's inner loop sets the same pairs on every call: nothing to rebuild or upload)
        std::vector<int> off, inc;
        gain_incidence(nant_, nbls_, ant1, ant2, off, inc);
        nbls = -1;
        h_ant1.assign(ant1, ant1 + nbls_);
        h_ant2.assign(ant2, ant2 + nbls_);
        const size_t nb = sizeof(int) * (size_t)nbls_;
        d_ant1.reserve(std::max<size_t>(nb, 16));
        d_ant2.reserve(std::max<size_t>(nb, 16));
        d_off.reserve(sizeof(int) * off.size());
        d_inc.reserve(std::max<size_t>(2 * nb, 16));
        if (nb) {
            FV_HIP(hipMemcpyAsync(d_ant1.p, ant1, nb, hipMemcpyHostToDevice, on));
            FV_HIP(hipMemcpyAsync(d_ant2.p, ant2, nb, hipMemcpyHostToDevice, on));
            FV_HIP(hipMemcpyAsync(d_inc.p, inc.data(), 2 * nb, hipMemcpyHostToDevice, on));
        }
        FV_HIP(hipMemcpyAsync(d_off.p, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, on));
        FV_HIP(hipStreamSynchronize(on));  // (off and inc are this call's)
        nant = nant_;
        nbls = nbls_;
    }
};

// ---------------------------------------------------------------------------------------------
// Jones gains (fv_jones_residual_chi2, fv_sim_run_residual_jones; DESIGN.md "Jones gains"): one 2 x 2 complex matrix per
// antenna in the data model of a polarized block.  The block, the pairs and the incidence lists are the gain kernels'
// above, tpol = 4: value pol nbls + k of a row is V[x, y] of baseline k = (a1, a2), pol = 2 x + y, y the feed of a1 (the
// conjugated antenna) and x of a2.  A row's matrices are 4 nant complex values of the run's precision,
// J[(2 i + j) nant + a] = Gamma_a[i, j], i the feed of the ideal antenna and j the measured one: antenna a's Jones matrix
// A_a[ax, feed] becomes A_a Gamma_a, and diagonal gains are Gamma_a = diag(g[a]).  With G1 = Gamma[a1], G2 = Gamma[a2],
//     V'[x, y]  = sum_{x', y'} conj(G1[y', y]) G2[x', x] V[x', y'],   delta = V' - d,   G'[x, y] = 2 w[x, y] delta[x, y],
//     G[x', y'] = sum_{x, y} conj(G2[x', x]) G'[x, y] G1[y', y]  (= d chi2 / dV),   row sum += w |delta|^2,
//     gjones[a, y', y] += sum_x conj(G'[x, y]) (G2^T V)[x, y']   for every k with a1[k] = a  (side 0),
//     gjones[a, x', x] += sum_y G'[x, y] conj((V conj G1)[x', y])  for every k with a2[k] = a  (side 1),
// d chi2 = Re sum conj(gjones) dGamma.  w == 0 flags that one (x, y) sample: G' = 0 exactly there, the datum is not used
// (a select), nothing is added to chi2 or gjones, and the baseline's other samples still use all four model values; a
// baseline with all four samples flagged stores G = 0 exactly.
//   Three kernels, no floating-point atomics.  k_jones_gradient runs first, while the block still holds V.
// k_jones_residual_rows follows, in place; the unit of its work is a baseline, whose four values are coupled: a thread takes
// a run of consecutive baselines in all four planes, as many as one 16-byte vector of a plane holds -- one in fp64, where
// every value is such a vector wherever the row starts, two in fp32 when every array is 16-byte aligned and nbls is even,
// so that the four planes are aligned alike in the block's own index; else, and for the clipped runs at a row's ends,
// baseline by baseline.  Consecutive lanes take consecutive runs: every access is coalesced.  A block takes
// RES_CHUNKS * 256 * RES_W<T> baselines.  The row's matrices are staged in dynamic LDS when they fit GAIN_LDS_BYTES.  In T every
// operation rounds on its own (no contraction), in this order, every sum of two products left to right:
//     B[x', y]  = V[x', 0] conj(G1[0, y]) + V[x', 1] conj(G1[1, y]),      V'[x, y]  = G2[0, x] B[0, y] + G2[1, x] B[1, y],
//     delta = V' - d,   G' = 2 (w delta),
//     C[x', y]  = conj(G2[x', 0]) G'[0, y] + conj(G2[x', 1]) G'[1, y],    G[x', y'] = C[x', 0] G1[y', 0] + C[x', 1] G1[y', 1],
// a complex product as (ar br - ai bi, ar bi + ai br) and a conj(b) as (ar br + ai bi, ai br - ar bi).  With identity
// matrices B = V' = V and G = G' exactly: k_residual_rows<T, false>'s bits.  A thread's baselines are not the row walk's
// chunks, so the row terms (row_term, 0 for a flagged sample) go to `terms`, an fp64 block in the block's own index, and
// k_jones_rows_sum adds them exactly as k_residual_rows adds its own -- per thread in chunk order, row_tail, then
// k_chi2_rows_reduce -- which makes chi2 the plain kernel's bit for bit whenever delta is.
template <typename T>
__device__ __forceinline__ cplx<T> jones_mul(const cplx<T> &a, const cplx<T> &b) {  // a b
#pragma clang fp contract(off)
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T>
__device__ __forceinline__ cplx<T> jones_mulc(const cplx<T> &a, const cplx<T> &b) {  // a conj(b)
#pragma clang fp contract(off)
    return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}
template <typename T>
__device__ __forceinline__ cplx<T> jones_add(const cplx<T> &a, const cplx<T> &b) {
#pragma clang fp contract(off)
    return {a.re + b.re, a.im + b.im};
}
// The stored G of one baseline from its G' (the Jones objective and the Gauss-Newton product with Jones gains share it):
//     C[x', y] = conj(G2[x', 0]) G'[0, y] + conj(G2[x', 1]) G'[1, y],    G[x', y'] = C[x', 0] G1[y', 0] + C[x', 1] G1[y', 1],
// every operation rounding on its own; `any` false (every sample flagged): exactly 0 whatever the matrices hold.
template <typename T>
__device__ __forceinline__ void jones_stored_g(const cplx<T> (&gp)[4], const cplx<T> (&g1)[4], const cplx<T> (&g2)[4], bool any,
                                               cplx<T> (&g_out)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int xs = 0; xs < 2; ++xs) {
        const cplx<T> c0 = jones_add(jones_mulc(gp[0], g2[2 * xs]), jones_mulc(gp[2], g2[2 * xs + 1]));
        const cplx<T> c1 = jones_add(jones_mulc(gp[1], g2[2 * xs]), jones_mulc(gp[3], g2[2 * xs + 1]));
#pragma unroll
        for (int ys = 0; ys < 2; ++ys) {
            const cplx<T> g = jones_add(jones_mul(c0, g1[2 * ys]), jones_mul(c1, g1[2 * ys + 1]));
            g_out[2 * xs + ys] = any ? g : cplx<T>{(T)0, (T)0};
        }
    }
}
// One baseline (a1, a2) in place: v[2 x + y] = V -> G, the row terms of its four samples, the counts of bad input.  J: the
// row's matrices (staged or global), entry [2 i + j] of antenna a at J[(2 i + j) nant + a].
template <typename T>
__device__ __forceinline__ void jones_residual_baseline(cplx<T> (&v)[4], const cplx<T> (&d)[4], const T (&w)[4],
                                                        const cplx<T> *J, int nant, int a1, int a2, double (&term)[4],
                                                        int &bad_w, int &bad_d) {
#pragma clang fp contract(off)
    const cplx<T> g1[4] = {J[a1], J[nant + a1], J[2 * nant + a1], J[3 * nant + a1]};
    const cplx<T> g2[4] = {J[a2], J[nant + a2], J[2 * nant + a2], J[3 * nant + a2]};
    cplx<T> b[4], gp[4];  // B[x', y] at [2 x' + y], G'[x, y] at [2 x + y]
#pragma unroll
    for (int xs = 0; xs < 2; ++xs)
#pragma unroll
        for (int y = 0; y < 2; ++y)
            b[2 * xs + y] = jones_add(jones_mulc(v[2 * xs], g1[y]), jones_mulc(v[2 * xs + 1], g1[2 + y]));
    bool any = false;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int s = 2 * x + y;
            const cplx<T> vp = jones_add(jones_mul(g2[x], b[y]), jones_mul(g2[2 + x], b[2 + y]));
            if (!(w[s] >= (T)0) || !isfinite(w[s])) ++bad_w;
            if (w[s] > (T)0) {
                if (!isfinite(d[s].re) || !isfinite(d[s].im)) ++bad_d;
                const T dr = vp.re - d[s].re, di = vp.im - d[s].im;
                gp[s] = {(T)2 * (w[s] * dr), (T)2 * (w[s] * di)};
                term[s] = row_term<T>(w[s], dr, di);
                any = true;
            } else {  // flagged (or counted above)
                gp[s] = {(T)0, (T)0};
                term[s] = 0.0;
            }
        }
    jones_stored_g<T>(gp, g1, g2, any, v);
}
// One baseline of a row: its four values at e, e + nbls, ... of the block's index.
template <typename T>
__device__ __forceinline__ void jones_residual_at(int64_t e, int nbls, int a1, int a2, const cplx<T> *J, int nant,
                                                  cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data,
                                                  const T *__restrict__ weights, double *__restrict__ terms, int &bad_w,
                                                  int &bad_d) {
    cplx<T> v[4], d[4];
    T w[4];
    double term[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        v[p] = vis[e + (int64_t)p * nbls];
        d[p] = data[e + (int64_t)p * nbls];
        w[p] = weights ? weights[e + (int64_t)p * nbls] : (T)1;
    }
    jones_residual_baseline<T>(v, d, w, J, nant, a1, a2, term, bad_w, bad_d);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        vis[e + (int64_t)p * nbls] = v[p];
        terms[e + (int64_t)p * nbls] = term[p];
    }
}
template <typename T>
__global__ void __launch_bounds__(256)
    k_jones_residual_rows(cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                          const cplx<T> *__restrict__ jones, const int *__restrict__ ant1, const int *__restrict__ ant2,
                          int64_t nrows, int nbls, int nant, int in_lds, int vec, double *__restrict__ terms,
                          int *__restrict__ bad) {
    constexpr int W = RES_W<T>;
    constexpr int R = 16 / (int)sizeof(cplx<T>);  // the baselines of one 16-byte vector of a plane: 1 (fp64) or 2 (fp32)
    extern __shared__ __align__(16) unsigned char gain_lds[];
    const int nj = 4 * nant;
    const int64_t L = 4 * (int64_t)nbls;
    // runs of R baselines, when the four planes of a run are aligned alike; else -- and always in fp64, where a value is a
    // 16-byte vector -- one baseline at a time.  Consecutive lanes take consecutive runs.
    const bool runs = R > 1 && vec && nbls % R == 0;
    const int step = runs ? R : 1, nit = RES_CHUNKS * W / step;
    int bad_w = 0, bad_d = 0;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *J = jones + row * nj;
        if (in_lds) {
            cplx<T> *jl = reinterpret_cast<cplx<T> *>(gain_lds);
            for (int i = threadIdx.x; i < nj; i += 256) jl[i] = J[i];
            J = jl;
            __syncthreads();
        }
        const int64_t lo = row * L;
        const int shift = runs ? (int)(lo % R) : 0;  // run r holds the baselines [r R - shift, r R - shift + R)
        const int64_t kblock = (int64_t)blockIdx.x * (RES_CHUNKS * 256 * W) - shift;
        for (int i = 0; i < nit; ++i) {
            const int64_t k0 = kblock + ((int64_t)i * 256 + threadIdx.x) * step;
            if (k0 >= nbls) break;
            if constexpr (R > 1) {
                if (runs && k0 >= 0 && k0 + R <= nbls) {
                    union {
                        uint4 q;
                        cplx<T> c[R];
                    } v[4], d[4];
                    T w[4][R];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int64_t e = lo + (int64_t)p * nbls + k0;
                        v[p].q = *reinterpret_cast<const uint4 *>(vis + e);
                        d[p].q = *reinterpret_cast<const uint4 *>(data + e);
#pragma unroll
                        for (int j = 0; j < R; ++j) w[p][j] = weights ? weights[e + j] : (T)1;
                    }
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        cplx<T> vv[4] = {v[0].c[j], v[1].c[j], v[2].c[j], v[3].c[j]};
                        const cplx<T> dd[4] = {d[0].c[j], d[1].c[j], d[2].c[j], d[3].c[j]};
                        const T w4[4] = {w[0][j], w[1][j], w[2][j], w[3][j]};
                        double term[4];
                        jones_residual_baseline<T>(vv, dd, w4, J, nant, ant1[k0 + j], ant2[k0 + j], term, bad_w, bad_d);
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            v[p].c[j] = vv[p];
                            terms[lo + (int64_t)p * nbls + k0 + j] = term[p];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) *reinterpret_cast<uint4 *>(vis + lo + (int64_t)p * nbls + k0) = v[p].q;
                    continue;
                }
            }
            const int64_t kb = k0 + step < nbls ? k0 + step : nbls;
            for (int64_t k = k0 > 0 ? k0 : 0; k < kb; ++k)
                jones_residual_at<T>(lo + k, nbls, ant1[k], ant2[k], J, nant, vis, data, weights, terms, bad_w, bad_d);
        }
        if (in_lds) __syncthreads();  // (the next row of this block stages its matrices again)
    }
    if (bad_w) atomicAdd(bad, bad_w);
    if (bad_d) atomicAdd(bad + 1, bad_d);
}
// The rows' sums of k_jones_residual_rows' terms, added as k_residual_rows adds its own: the row walk's chunks, per thread
// in chunk order, then row_tail.  partials[row][block] as there.
template <typename T>
__global__ void __launch_bounds__(256)
    k_jones_rows_sum(const double *__restrict__ terms, int64_t nrows, int64_t L, double *__restrict__ partials,
                     int *__restrict__ bad) {
    constexpr int W = RES_W<T>;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const int64_t lo = row * L, hi = lo + L, c0 = lo / W;
        double s = 0.0;
        for (int i = 0; i < RES_CHUNKS; ++i) {
            const RowChunk c = row_chunk<T>(c0, lo, hi, i, 0);
            if (c.e0 >= hi) break;
            for (int64_t e = c.a; e < c.b; ++e) s += terms[e];
        }
        row_tail(s, 0, 0, row, partials, bad);
    }
}
// gjones[((row 2 + i) 2 + j) nant + a]: one wave per (row, antenna), all four entries of the antenna's matrix in fp64 (8
// doubles per lane), so each incident baseline's four samples are read once per side.  Lane l takes the entries l, l + 64,
// ... of the antenna's incidence list in order; everything is formed in fp64 from the T-typed inputs; an __shfl_xor tree;
// an antenna without a baseline gets exactly 0.  vis still holds V.
template <typename T>
__global__ void __launch_bounds__(256)
    k_jones_gradient(const cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                     const cplx<T> *__restrict__ jones, const int *__restrict__ ant1, const int *__restrict__ ant2,
                     const int *__restrict__ inc_off, const int *__restrict__ inc, int64_t nrows, int nbls, int nant,
                     cplx<double> *__restrict__ gjones) {
    const int ant = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (ant >= nant) return;  // (whole waves: the tree below stays inside one)
    const int i0 = inc_off[ant], i1 = inc_off[ant + 1];
    const int64_t L = 4 * (int64_t)nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *J = jones + row * 4 * nant;
        cplx<double> acc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            const int64_t e = row * L + k;
            cplx<double> v[4], g1[4], g2[4], m[4], gp[4];
            double w2[4];
            bool any = false;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const T wt = weights ? weights[e + (int64_t)p * nbls] : (T)1;
                w2[p] = wt > (T)0 ? 2.0 * (double)wt : 0.0;
                any = any || wt > (T)0;
            }
            if (!any) continue;  // every sample flagged: nothing is added, nothing more is read
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                v[p] = {(double)vis[e + (int64_t)p * nbls].re, (double)vis[e + (int64_t)p * nbls].im};
                g1[p] = {(double)J[p * nant + a1].re, (double)J[p * nant + a1].im};
                g2[p] = {(double)J[p * nant + a2].re, (double)J[p * nant + a2].im};
            }
            // side 0: M[x, y'] = (G2^T V)[x, y'] at [2 x + y'], V'[x, y] = sum_y' M[x, y'] conj(G1[y', y]);
            // side 1: M[x', y] = (V conj G1)[x', y] at [2 x' + y], V'[x, y] = sum_x' G2[x', x] M[x', y]
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    m[2 * r + c] = side ? cadd(cmul(v[2 * r], cconj(g1[c])), cmul(v[2 * r + 1], cconj(g1[2 + c])))
                                        : cadd(cmul(g2[r], v[c]), cmul(g2[2 + r], v[2 + c]));
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const int s = 2 * x + y;
                    gp[s] = {0.0, 0.0};
                    if (w2[s] > 0.0) {  // (a flagged datum is not read)
                        const cplx<double> vp = side ? cadd(cmul(g2[x], m[y]), cmul(g2[2 + x], m[2 + y]))
                                                     : cadd(cmul(m[2 * x], cconj(g1[y])), cmul(m[2 * x + 1], cconj(g1[2 + y])));
                        gp[s] = {w2[s] * (vp.re - (double)data[e + (int64_t)s * nbls].re),
                                 w2[s] * (vp.im - (double)data[e + (int64_t)s * nbls].im)};
                    }
                }
            // side 0: acc[y', y] += sum_x conj(G'[x, y]) M[x, y'];  side 1: acc[x', x] += sum_y G'[x, y] conj(M[x', y])
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const cplx<double> t = side ? cadd(cmul(gp[2 * c], cconj(m[2 * r])), cmul(gp[2 * c + 1], cconj(m[2 * r + 1])))
                                                : cadd(cmul(cconj(gp[c]), m[r]), cmul(cconj(gp[2 + c]), m[2 + r]));
                    acc[2 * r + c].re += t.re;
                    acc[2 * r + c].im += t.im;
                }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            for (int off = 32; off > 0; off >>= 1) {
                acc[s].re += __shfl_xor(acc[s].re, off, 64);
                acc[s].im += __shfl_xor(acc[s].im, off, 64);
            }
            if (lane == 0) gjones[(row * 4 + s) * nant + ant] = acc[s];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Gain solve on a resident model (fv_gain_normal_rows, fv_gain_solve; DESIGN.md "Gain solve").  The block, the pairs, the
// feeds and the incidence lists are the gain kernels' above; V, d and w are read only.  The iterate is complex128
// whatever T is: (nunits, nfeed nant), row `row` reads unit row / rows_per_unit (a unit is a frequency for time-constant
// gains, rows_per_unit = ntimes, and a row for per-time gains).  A sample is used when w > 0 and a1 != a2; a flagged
// sample is skipped before V and d are read.  For fixed V the least-squares problem in one antenna's gain, the others
// held, is linear; its normal sums per (row, feed f, antenna a) are
//     side 0 (a = a1, f = p, every q):  num += w g[q, a2] V conj(d),   den += w |g[q, a2]|^2 |V|^2
//     side 1 (a = a2, f = q, every p):  num += w g[p, a1] conj(V) d,   den += w |g[p, a1]|^2 |V|^2
// and with autos flagged ggains = 2 (den g - num).  k_gain_normal is k_gain_gradient's gather: one wave per (row, feed,
// antenna), lane l takes the entries l, l + 64, ... in order, every term formed and added in fp64, an __shfl_xor tree,
// one complex128 and one float64 per wave; the row's gains are staged in LDS when they fit GAIN_LDS_BYTES (a wave reads
// the other antennas' at random), which is why a wave without an antenna stays for the barriers instead of leaving.
// CHI2 = true writes instead the wave's sum of w |conj(g[p, a1]) g[q, a2] V - d|^2 over its side-0 entries -- every
// baseline once -- into part[(row nfeed + feed) nant + a]; k_gain_chi2_rows adds a row's, a wave per row in a fixed order.
// k_gain_update, one block per unit: the sums of the unit's rows in ascending order, g^ = num / den where den > 0 (else
// the antenna keeps its value and is not solved), g <- g^ on odd iterations and (g^ + g) / 2 on even ones, written into
// the OTHER buffer, and change[unit] = max |g_new - g| / max |g_new| (a max: any order gives the same bits).  No
// floating-point atomics anywhere.
// GROUPED = true is the gather of the redundant solve below: the model of baseline k is its group's visibility,
// uvis[(row tpol + pol) ngroups + group[k]] (complex128 whatever T is), read in place of vis[e]; nothing else differs.
template <typename T, bool CHI2, bool GROUPED = false>
__global__ void __launch_bounds__(256)
    k_gain_normal(const cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                  const cplx<double> *__restrict__ gains, const int *__restrict__ ant1, const int *__restrict__ ant2,
                  const int *__restrict__ inc_off, const int *__restrict__ inc, int64_t nrows, int64_t rows_per_unit, int nbls,
                  int tpol, int nant, int in_lds, cplx<double> *__restrict__ num, double *__restrict__ den,
                  const cplx<double> *__restrict__ uvis = nullptr, const int *__restrict__ group = nullptr, int ngroups = 0) {
    extern __shared__ __align__(16) unsigned char gain_lds[];
    const int nfeed = tpol == 4 ? 2 : 1, ng = nfeed * nant;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const bool active = wave < ng;  // (whole waves: the tree below stays inside one)
    const int feed = active ? wave / nant : 0, ant = active ? wave - feed * nant : 0;
    const int i0 = active ? inc_off[ant] : 0, i1 = active ? inc_off[ant + 1] : 0;
    const int64_t L = (int64_t)tpol * nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<double> *g = gains + (row / rows_per_unit) * ng;
        if (in_lds) {
            cplx<double> *gl = reinterpret_cast<cplx<double> *>(gain_lds);
            for (int i = threadIdx.x; i < ng; i += 256) gl[i] = g[i];
            g = gl;
            __syncthreads();
        }
        double sr = 0.0, si = 0.0, sd = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            if (a1 == a2 || (CHI2 && side)) continue;  // an auto-correlation is flagged; chi2 counts a baseline once
            for (int o = 0; o < nfeed; ++o) {          // the other antenna's feed
                const int p = side ? o : feed, q = side ? feed : o;
                const int64_t e = row * L + (int64_t)(nfeed == 2 ? 2 * q + p : 0) * nbls + k;
                const T wt = weights ? weights[e] : (T)1;
                if (!(wt > (T)0)) continue;  // flagged: nothing is added, V and the datum are not read
                const cplx<double> go = side ? g[p * nant + a1] : g[q * nant + a2];  // the other antenna's gain
                cplx<double> v;
                if (GROUPED)
                    v = uvis[(row * tpol + (nfeed == 2 ? 2 * q + p : 0)) * ngroups + group[k]];
                else
                    v = {(double)vis[e].re, (double)vis[e].im};
                const cplx<double> d = {(double)data[e].re, (double)data[e].im};
                if (CHI2) {
                    const cplx<double> vp = cmul(cmul(cconj(g[feed * nant + ant]), go), v);
                    const double dr = vp.re - d.re, di = vp.im - d.im;
                    sd += (double)wt * (dr * dr + di * di);
                } else {
                    // side 0: g2 V conj(d);  side 1: g1 conj(V) d
                    const cplx<double> t = side ? cmul(cmul(go, cconj(v)), d) : cmul(cmul(go, v), cconj(d));
                    sr += (double)wt * t.re;
                    si += (double)wt * t.im;
                    sd += (double)wt * ((go.re * go.re + go.im * go.im) * (v.re * v.re + v.im * v.im));
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            if (!CHI2) {
                sr += __shfl_xor(sr, off, 64);
                si += __shfl_xor(si, off, 64);
            }
            sd += __shfl_xor(sd, off, 64);
        }
        if (active && lane == 0) {
            const int64_t at = (row * nfeed + feed) * nant + ant;
            if (!CHI2) num[at] = {sr, si};
            den[at] = sd;
        }
        if (in_lds) __syncthreads();  // (the next row of this block stages its gains again)
    }
}
// One block per solve unit; see above.  num, den: (nunits rows_per_unit, ng); g_old, g_new: (nunits, ng), two buffers;
// odd: the iteration's parity; solved[unit ng + i] = den > 0.
__global__ void __launch_bounds__(256)
    k_gain_update(const cplx<double> *__restrict__ num, const double *__restrict__ den, const cplx<double> *__restrict__ g_old,
                  cplx<double> *__restrict__ g_new, int64_t rows_per_unit, int ng, int odd, double *__restrict__ change,
                  int *__restrict__ solved) {
    __shared__ double wave_max[2][4];
    const int64_t unit = blockIdx.x;
    double md = 0.0, mn = 0.0;  // max |g_new - g|^2, max |g_new|^2 (the square root is monotone: taken once, at the end)
    for (int i = threadIdx.x; i < ng; i += 256) {
        double nr = 0.0, ni = 0.0, dn = 0.0;
        for (int64_t r = 0; r < rows_per_unit; ++r) {  // ascending time
            const int64_t at = (unit * rows_per_unit + r) * ng + i;
            nr += num[at].re;
            ni += num[at].im;
            dn += den[at];
        }
        const cplx<double> g = g_old[unit * ng + i];
        cplx<double> gn = g;
        if (dn > 0.0) {
            gn = {nr / dn, ni / dn};
            if (!odd) gn = {0.5 * (gn.re + g.re), 0.5 * (gn.im + g.im)};
        }
        g_new[unit * ng + i] = gn;
        solved[unit * ng + i] = dn > 0.0 ? 1 : 0;
        const double dr = gn.re - g.re, di = gn.im - g.im;
        md = fmax(md, dr * dr + di * di);
        mn = fmax(mn, gn.re * gn.re + gn.im * gn.im);
    }
    for (int off = 32; off > 0; off >>= 1) {
        md = fmax(md, __shfl_xor(md, off, 64));
        mn = fmax(mn, __shfl_xor(mn, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        wave_max[0][threadIdx.x >> 6] = md;
        wave_max[1][threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        md = fmax(fmax(wave_max[0][0], wave_max[0][1]), fmax(wave_max[0][2], wave_max[0][3]));
        mn = fmax(fmax(wave_max[1][0], wave_max[1][1]), fmax(wave_max[1][2], wave_max[1][3]));
        change[unit] = mn > 0.0 ? sqrt(md) / sqrt(mn) : 0.0;
    }
}
// chi2_rows[row] = the sum of a row's n partials of the chi2 pass (n = nfeed nant: hundreds, where k_chi2_rows_reduce's one
// thread per row would run as many dependent adds): one wave per row, lane l adds the partials l, l + 64, ... in order,
// then an __shfl_xor tree -- a fixed order, the same bits on every run.
__global__ void __launch_bounds__(256)
    k_gain_chi2_rows(const double *__restrict__ part, int64_t nrows, int n, double *__restrict__ chi2_rows) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (row >= nrows) return;  // (whole waves)
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += part[row * n + i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) chi2_rows[row] = s;
}
// The counting pass of a solve: bad[0] weights that are negative or not finite, bad[1] data that are not finite at a
// used sample (w > 0, a1 != a2), bad[2] model values that are not finite (vis null: a solve without a model, nothing is
// counted there).  n = nrows tpol nbls elements, read only.
template <typename T>
__global__ void __launch_bounds__(256)
    k_gain_solve_check(const cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                       const int *__restrict__ ant1, const int *__restrict__ ant2, int64_t n, int nbls, int *__restrict__ bad) {
    int bad_w = 0, bad_d = 0, bad_v = 0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int k = (int)(e % nbls);
        const T w = weights ? weights[e] : (T)1;
        if (!(w >= (T)0) || !isfinite(w)) ++bad_w;
        if (w > (T)0 && ant1[k] != ant2[k] && (!isfinite(data[e].re) || !isfinite(data[e].im))) ++bad_d;
        if (vis && (!isfinite(vis[e].re) || !isfinite(vis[e].im))) ++bad_v;
    }
    if (bad_w) atomicAdd(bad, bad_w);
    if (bad_d) atomicAdd(bad + 1, bad_d);
    if (bad_v) atomicAdd(bad + 2, bad_v);
}
// Queues one evaluation of the normal sums (num, den: (nrows, ng)) or, with chi2_part, of the chi2 partials on `on`.
// All device pointers; weights may be null.
template <typename T>
inline void launch_gain_normal(hipStream_t on, const cplx<T> *vis, const cplx<T> *data, const T *weights, const cplx<double> *gains,
                               const GainPairs &gp, int64_t nrows, int64_t rows_per_unit, int tpol, cplx<double> *num, double *den,
                               double *chi2_part) {
    const int nbls = (int)gp.nbls, nant = gp.nant, ng = (tpol == 4 ? 2 : 1) * nant;
    const size_t lds = sizeof(cplx<double>) * (size_t)ng;
    const int in_lds = lds <= GAIN_LDS_BYTES;
    const dim3 grid((unsigned)cdiv(ng, 4), (unsigned)std::min<int64_t>(nrows, 65535));
    if (chi2_part)
        hipLaunchKernelGGL((k_gain_normal<T, true>), grid, dim3(256), in_lds ? lds : 0, on, vis, data, weights, gains,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, tpol, nant, in_lds, (cplx<double> *)nullptr, chi2_part);
    else
        hipLaunchKernelGGL((k_gain_normal<T, false>), grid, dim3(256), in_lds ? lds : 0, on, vis, data, weights, gains,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, tpol, nant, in_lds, num, den);
}
// the message of a solve that met bad input (k_gain_solve_check's counters)
inline void throw_if_bad_solve_input(const int bad[3]) {
    throw_if_bad_residual_input(bad);
    if (bad[2]) throw Error(FV_ERR_ARG, std::to_string(bad[2]) + " values of the model are not finite");
}

// ---------------------------------------------------------------------------------------------
// Redundant solve (fv_redundant_vis_rows, fv_redundant_normal_rows, fv_redundant_solve; DESIGN.md "Redundant solve"):
// the gain solve above without a sky.  Every baseline k belongs to a redundant group, group[k] in [0, ngroups), and the
// model is V'[row, pol, k] = conj(g[p, a1]) g[q, a2] U[row, pol, group[k]] with one unknown visibility U per (row, pol,
// group), complex128 whatever T is.  The solve alternates two linear problems.  For fixed gains the best U is a weighted
// average over the group's used samples (w > 0, a1 != a2; a flagged datum is not read): with m = conj(g[p, a1]) g[q, a2]
//     num = sum w conj(m) d,   den = sum w |m|^2,   U = num / den where den > 0, else U keeps its value,
// k_red_vis.  For fixed U the gains are the gain solve's with V = U[group[k]]: k_gain_normal<T, CHI2, true> and
// k_gain_update as it stands.  The groups' members come as a CSR, goff[r] .. goff[r + 1] the baselines of group r in
// ascending order (group_members): one wave per (row, group), lane l takes the members l, l + 64, ... in order and all tpol
// samples of a member -- tpol complex num and tpol den in fp64 registers, every term formed in fp64 from the T-typed inputs
// --, an __shfl_xor tree, and lane 0 writes U and den.  The row's gains are staged in LDS when they fit GAIN_LDS_BYTES, which
// is why a wave without a group stays for the barriers.  With the baselines in group order a group's members are
// consecutive and the loads of d and w coalesce.  No floating-point atomics: the same input gives the same bits.
inline void group_members(int ngroups, int64_t nbls, const int *group, std::vector<int> &off, std::vector<int> &mem) {
    FV_REQUIRE(ngroups >= 1 && nbls >= 0 && nbls < ((int64_t)1 << 30) && (nbls == 0 || group), "groups: bad ngroups, nbls or null group");
    for (int64_t k = 0; k < nbls; ++k) FV_REQUIRE(group[k] >= 0 && group[k] < ngroups, "groups: group index outside [0, ngroups)");
    off.assign((size_t)ngroups + 1, 0);
    for (int64_t k = 0; k < nbls; ++k) ++off[group[k] + 1];
    for (int r = 0; r < ngroups; ++r) off[r + 1] += off[r];
    mem.assign((size_t)nbls, 0);
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int64_t k = 0; k < nbls; ++k) mem[at[group[k]]++] = (int)k;
}
// The group of every baseline and the groups' member lists on the device (one set per call)
struct RedGroups {
    DevBuf d_group, d_off, d_mem;
    int ngroups = 0;
    int64_t nbls = -1;         // -1: not set
    std::vector<int> h_group;  // what the device holds while nbls >= 0
    void set(hipStream_t on, int ngroups_, int64_t nbls_, const int *group) {
        if (nbls >= 0 && nbls_ == nbls && ngroups_ == ngroups && (nbls_ == 0 || group) && std::equal(h_group.begin(), h_group.end(), group))
            return;
        std::vector<int> off, mem;
        group_members(ngroups_, nbls_, group, off, mem);
        nbls = -1;
        h_group.assign(group, group + nbls_);
        const size_t nb = sizeof(int) * (size_t)nbls_;
        d_group.reserve(std::max<size_t>(nb, 16));
        d_mem.reserve(std::max<size_t>(nb, 16));
        d_off.reserve(sizeof(int) * off.size());
        if (nb) {
            FV_HIP(hipMemcpyAsync(d_group.p, group, nb, hipMemcpyHostToDevice, on));
            FV_HIP(hipMemcpyAsync(d_mem.p, mem.data(), nb, hipMemcpyHostToDevice, on));
        }
        FV_HIP(hipMemcpyAsync(d_off.p, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, on));
        FV_HIP(hipStreamSynchronize(on));  // (off and mem are this call's)
        ngroups = ngroups_;
        nbls = nbls_;
    }
};
// uvis, den: (nrows, TPOL, ngroups); den may be null.  TPOL is the template's so that the sums stay in registers.  LANES
// lanes take a group: 64, a wave, or 16 (-DFV_RED_VIS_LANES=16: four groups per wave, lane l of a group's 16 takes the
// members l, l + 16, ...; measured on HERA-350, whose median group has 3 members, in profiles/MEASUREMENTS.md).
#ifndef FV_RED_VIS_LANES
#define FV_RED_VIS_LANES 64
#endif
template <typename T, int TPOL, int LANES>
__global__ void __launch_bounds__(256)
    k_red_vis(const cplx<T> *__restrict__ data, const T *__restrict__ weights, const cplx<double> *__restrict__ gains,
              const int *__restrict__ ant1, const int *__restrict__ ant2, const int *__restrict__ goff, const int *__restrict__ gmem,
              int64_t nrows, int64_t rows_per_unit, int nbls, int nant, int ngroups, int in_lds, cplx<double> *__restrict__ uvis,
              double *__restrict__ den) {
    extern __shared__ __align__(16) unsigned char gain_lds[];
    constexpr int nfeed = TPOL == 4 ? 2 : 1;
    const int ng = nfeed * nant;
    static_assert(LANES == 64 || LANES == 16, "a group takes a wave or a quarter of one");
    const int r = (int)blockIdx.x * (256 / LANES) + (int)(threadIdx.x / LANES), lane = (int)(threadIdx.x % LANES);
    const bool active = r < ngroups;  // (whole waves stay: the tree below is inside a group's aligned LANES lanes)
    const int i0 = active ? goff[r] : 0, i1 = active ? goff[r + 1] : 0;
    const int64_t L = (int64_t)TPOL * nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<double> *g = gains + (row / rows_per_unit) * ng;
        if (in_lds) {
            cplx<double> *gl = reinterpret_cast<cplx<double> *>(gain_lds);
            for (int i = threadIdx.x; i < ng; i += 256) gl[i] = g[i];
            g = gl;
            __syncthreads();
        }
        double sr[TPOL], si[TPOL], sd[TPOL];
#pragma unroll
        for (int pol = 0; pol < TPOL; ++pol) sr[pol] = si[pol] = sd[pol] = 0.0;
        for (int i = i0 + lane; i < i1; i += LANES) {
            const int k = gmem[i];
            const int a1 = ant1[k], a2 = ant2[k];
            if (a1 == a2) continue;  // an auto-correlation is flagged
#pragma unroll
            for (int pol = 0; pol < TPOL; ++pol) {
                const int p = pol & 1, q = pol >> 1;
                const int64_t e = row * L + (int64_t)pol * nbls + k;
                const T wt = weights ? weights[e] : (T)1;
                if (!(wt > (T)0)) continue;  // flagged: nothing is added, the datum is not read
                const cplx<double> m = cmul(cconj(g[p * nant + a1]), g[q * nant + a2]);
                const cplx<double> d = {(double)data[e].re, (double)data[e].im};
                const cplx<double> t = cmul(cconj(m), d);
                sr[pol] += (double)wt * t.re;
                si[pol] += (double)wt * t.im;
                sd[pol] += (double)wt * (m.re * m.re + m.im * m.im);
            }
        }
#pragma unroll
        for (int pol = 0; pol < TPOL; ++pol)
            for (int off = LANES / 2; off > 0; off >>= 1) {
                sr[pol] += __shfl_xor(sr[pol], off, 64);
                si[pol] += __shfl_xor(si[pol], off, 64);
                sd[pol] += __shfl_xor(sd[pol], off, 64);
            }
        if (active && lane == 0) {
#pragma unroll
            for (int pol = 0; pol < TPOL; ++pol) {
                const int64_t at = (row * TPOL + pol) * ngroups + r;
                if (sd[pol] > 0.0) uvis[at] = {sr[pol] / sd[pol], si[pol] / sd[pol]};
                if (den) den[at] = sd[pol];
            }
        }
        if (in_lds) __syncthreads();  // (the next row of this block stages its gains again)
    }
}
// Queues one U-step on `on`.  All device pointers; weights and den may be null.
template <typename T>
inline void launch_red_vis(hipStream_t on, const cplx<T> *data, const T *weights, const cplx<double> *gains, const GainPairs &gp,
                           const RedGroups &rg, int64_t nrows, int64_t rows_per_unit, int tpol, cplx<double> *uvis, double *den) {
    const int nbls = (int)gp.nbls, nant = gp.nant, ng = (tpol == 4 ? 2 : 1) * nant;
    const size_t lds = sizeof(cplx<double>) * (size_t)ng;
    const int in_lds = lds <= GAIN_LDS_BYTES;
    const dim3 grid((unsigned)cdiv(rg.ngroups, 256 / FV_RED_VIS_LANES), (unsigned)std::min<int64_t>(nrows, 65535));
    if (tpol == 4)
        hipLaunchKernelGGL((k_red_vis<T, 4, FV_RED_VIS_LANES>), grid, dim3(256), in_lds ? lds : 0, on, data, weights, gains, gp.d_ant1.as<int>(),
                           gp.d_ant2.as<int>(), rg.d_off.as<int>(), rg.d_mem.as<int>(), nrows, rows_per_unit, nbls, nant, rg.ngroups,
                           in_lds, uvis, den);
    else
        hipLaunchKernelGGL((k_red_vis<T, 1, FV_RED_VIS_LANES>), grid, dim3(256), in_lds ? lds : 0, on, data, weights, gains, gp.d_ant1.as<int>(),
                           gp.d_ant2.as<int>(), rg.d_off.as<int>(), rg.d_mem.as<int>(), nrows, rows_per_unit, nbls, nant, rg.ngroups,
                           in_lds, uvis, den);
}
// launch_gain_normal with the groups' visibilities as the model (k_gain_normal<T, CHI2, true>)
template <typename T>
inline void launch_red_normal(hipStream_t on, const cplx<double> *uvis, const cplx<T> *data, const T *weights,
                              const cplx<double> *gains, const GainPairs &gp, const RedGroups &rg, int64_t nrows,
                              int64_t rows_per_unit, int tpol, cplx<double> *num, double *den, double *chi2_part) {
    const int nbls = (int)gp.nbls, nant = gp.nant, ng = (tpol == 4 ? 2 : 1) * nant;
    const size_t lds = sizeof(cplx<double>) * (size_t)ng;
    const int in_lds = lds <= GAIN_LDS_BYTES;
    const dim3 grid((unsigned)cdiv(ng, 4), (unsigned)std::min<int64_t>(nrows, 65535));
    const cplx<T> *no_vis = nullptr;
    if (chi2_part)
        hipLaunchKernelGGL((k_gain_normal<T, true, true>), grid, dim3(256), in_lds ? lds : 0, on, no_vis, data, weights, gains,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, tpol, nant, in_lds, (cplx<double> *)nullptr, chi2_part, uvis, rg.d_group.as<int>(), rg.ngroups);
    else
        hipLaunchKernelGGL((k_gain_normal<T, false, true>), grid, dim3(256), in_lds ? lds : 0, on, no_vis, data, weights, gains,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, tpol, nant, in_lds, num, den, uvis, rg.d_group.as<int>(), rg.ngroups);
}

// ---------------------------------------------------------------------------------------------
// Firstcal (fv_firstcal_pair_delays, fv_firstcal_offsets; DESIGN.md "Firstcal"): the start of the redundant solve above, one
// delay and one complex number per antenna and feed, g[a](f) = c[a] exp(i s[a] (f - (nfreqs - 1) / 2)), s = 2 pi tau dnu.
// Stage 1, the pair delays.  A pair is two baselines k = pair1[i], k' = pair2[i] of one redundant group; feed p reads the
// parallel hand pol = 3 p of a polarized block.  The group's visibility cancels out of
//     z[feed, i, f] = sum_t d[f, t, pol, k] conj(d[f, t, pol, k'])   over the times at which both samples are used
// (w > 0 and a1 != a2: weights act as flags here, a flagged datum is not read), whose phase is linear in f with the slope
// s[a2[k]] - s[a1[k]] - s[a2[k']] + s[a1[k']].  k_firstcal_products: one thread per (feed, f, pair), the pair fastest, so
// that with the baselines in group order -- a pair is two neighbours -- the loads of d and w coalesce; every term formed and
// added in fp64, times ascending.  k_firstcal_delay: one wave per (feed, pair) finds the peak of the periodogram
//     P[n] = sum_f z[f] tw[(n f) mod ND],   tw[j] = exp(-2 pi i j / ND),   ND = pad nfreqs,   n = 0 .. ND - 1:
// lane l takes the bins l, l + 64, ... with the index n f mod ND advanced by n per channel (n < ND: one conditional
// subtraction, no product that could overflow), keeps the first maximum of |P[n]|^2 it meets, and an __shfl_xor tree takes
// the larger power, the lower bin on a tie.  The bin is signed, n - ND where 2 n >= ND.  Four rounds of a parabola through
// |P(x)|^2 at x - h, x, x + h, h = 1, 1/4, 1/16, 1/64, refine it: P(x) = sum_f z[f] exp(-2 pi i x f / ND) evaluated at the
// continuous x with sincospi in fp64, lane l adding the channels l, l + 64, ... of the three points, an __shfl_xor tree
// (every lane ends with the same bits), den = y- - 2 y0 + y+, and where den < 0 the step 0.5 h (y- - y+) / den clipped to
// +-h.  The wave's z row is staged in LDS when the block's four rows fit GAIN_LDS_BYTES, which is why a wave without a pair
// stays for the barrier.  A pair is used when at least two channels have a non-zero z; one that is not reports bin 0,
// x = 0 and power 0.  Stage 2 derotates the block by the delay model, k_firstcal_derotate,
//     d'[f, t, pol, k] = d exp(-i (f - (nfreqs - 1) / 2) (s[q, a2] - s[p, a1])),   p = pol & 1, q = pol >> 1,
// phase and product in fp64, into a buffer of the call (0 where the sample is not used: a flagged datum is not read), and
// the redundant solve runs on d' with the whole block as one unit.  No floating-point atomics: the same input gives the
// same bits.
template <typename T>
__global__ void __launch_bounds__(256)
    k_firstcal_products(const cplx<T> *__restrict__ data, const T *__restrict__ weights, const int *__restrict__ ant1,
                        const int *__restrict__ ant2, const int *__restrict__ pair1, const int *__restrict__ pair2, int nfreqs,
                        int ntimes, int nbls, int tpol, int npairs, cplx<double> *__restrict__ z) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= npairs) return;
    const int k1 = pair1[i], k2 = pair2[i];
    const bool cross = ant1[k1] != ant2[k1] && ant1[k2] != ant2[k2];  // an auto-correlation is flagged
    const int nfeed = tpol == 4 ? 2 : 1;
    for (int r = (int)blockIdx.y; r < nfeed * nfreqs; r += (int)gridDim.y) {
        const int f = r % nfreqs, feed = r / nfreqs;
        double sr = 0.0, si = 0.0;
        for (int t = 0; cross && t < ntimes; ++t) {  // ascending time
            const int64_t at = (((int64_t)f * ntimes + t) * tpol + 3 * feed) * nbls;
            if (weights && !(weights[at + k1] > (T)0 && weights[at + k2] > (T)0)) continue;  // flagged: the data are not read
            const cplx<double> a = {(double)data[at + k1].re, (double)data[at + k1].im};
            const cplx<double> b = {(double)data[at + k2].re, (double)data[at + k2].im};
            sr += a.re * b.re + a.im * b.im;
            si += a.im * b.re - a.re * b.im;
        }
        z[((int64_t)feed * npairs + i) * nfreqs + f] = {sr, si};
    }
}
// |P(x)|^2 at x - h, x and x + h for the continuous bin x: the wave's lanes split the channels; every lane returns the same bits
__device__ inline void firstcal_three_points(const cplx<double> *__restrict__ zr, int nfreqs, int lane, double x, double h, double nd,
                                             double y[3]) {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int f = lane; f < nfreqs; f += 64) {
        const cplx<double> zf = zr[f];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double sn, cs;
            sincospi(-2.0 * (x + (j - 1) * h) * (double)f / nd, &sn, &cs);
            s[2 * j] += zf.re * cs - zf.im * sn;
            s[2 * j + 1] += zf.re * sn + zf.im * cs;
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_xor(s[j], off, 64);
#pragma unroll
    for (int j = 0; j < 3; ++j) y[j] = s[2 * j] * s[2 * j] + s[2 * j + 1] * s[2 * j + 1];
}
// z: (nrows, nfreqs), nrows = nfeed npairs; tw: (nd); the outputs: (nrows).  Dynamic LDS: 4 nfreqs complex128 when in_lds.
__global__ void __launch_bounds__(256)
    k_firstcal_delay(const cplx<double> *__restrict__ z, const cplx<double> *__restrict__ tw, int nrows, int nfreqs, int nd, int in_lds,
                     int *__restrict__ peak_bin, double *__restrict__ delay_bins, double *__restrict__ power, double *__restrict__ total,
                     int *__restrict__ used) {
    extern __shared__ __align__(16) unsigned char gain_lds[];
    const int w = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int row = (int)blockIdx.x * 4 + w;
    const bool active = row < nrows;  // (whole waves: the trees below stay inside one)
    const cplx<double> *zr = z + (int64_t)(active ? row : 0) * nfreqs;
    double tot = 0.0;
    int nonzero = 0;
    for (int f = lane; active && f < nfreqs; f += 64) {
        const cplx<double> zf = zr[f];
        if (in_lds) reinterpret_cast<cplx<double> *>(gain_lds)[w * nfreqs + f] = zf;
        tot += zf.re * zf.re + zf.im * zf.im;
        nonzero += (zf.re != 0.0 || zf.im != 0.0) ? 1 : 0;
    }
    if (in_lds) {
        __syncthreads();
        zr = reinterpret_cast<const cplx<double> *>(gain_lds) + w * nfreqs;
    }
    for (int off = 32; off > 0; off >>= 1) {
        tot += __shfl_xor(tot, off, 64);
        nonzero += __shfl_xor(nonzero, off, 64);
    }
    if (!active) return;  // (no barrier follows)
    if (nonzero < 2) {
        if (lane == 0) {
            peak_bin[row] = 0;
            delay_bins[row] = 0.0;
            power[row] = 0.0;
            total[row] = tot;
            used[row] = 0;
        }
        return;
    }
    // the coarse peak: the first maximum of this lane's bins, then the wave's
    double best = -1.0;
    int best_n = 0;
    for (int n = lane; n < nd; n += 64) {
        double pr = 0.0, pi = 0.0;
        int j = 0;  // n f mod nd
        for (int f = 0; f < nfreqs; ++f) {
            const cplx<double> zf = zr[f], t = tw[j];
            pr += zf.re * t.re - zf.im * t.im;
            pi += zf.re * t.im + zf.im * t.re;
            j += n;
            if (j >= nd) j -= nd;
        }
        const double y = pr * pr + pi * pi;
        if (y > best) {
            best = y;
            best_n = n;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int on = __shfl_xor(best_n, off, 64);
        if (ob > best || (ob == best && on < best_n)) {
            best = ob;
            best_n = on;
        }
    }
    const int bin = 2 * best_n >= nd ? best_n - nd : best_n;
    double x = (double)bin, y[3];
    for (int round = 0; round < 4; ++round) {
        const double h = 1.0 / (double)(1 << (2 * round));
        firstcal_three_points(zr, nfreqs, lane, x, h, (double)nd, y);
        const double den = y[0] - 2.0 * y[1] + y[2];
        if (den < 0.0) x += fmin(fmax(0.5 * h * (y[0] - y[2]) / den, -h), h);
    }
    firstcal_three_points(zr, nfreqs, lane, x, 0.0, (double)nd, y);
    if (lane == 0) {
        peak_bin[row] = bin;
        delay_bins[row] = x;
        power[row] = y[1];
        total[row] = tot;
        used[row] = 1;
    }
}
// slopes: (nfeed, nant) radians per channel; out: the block's shape.  n = nfreqs ntimes tpol nbls elements.
template <typename T>
__global__ void __launch_bounds__(256)
    k_firstcal_derotate(const cplx<T> *__restrict__ data, const T *__restrict__ weights, const int *__restrict__ ant1,
                        const int *__restrict__ ant2, const double *__restrict__ slopes, int64_t n, int nfreqs, int ntimes, int nbls,
                        int tpol, int nant, cplx<T> *__restrict__ out) {
    const int64_t row_len = (int64_t)tpol * nbls;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / row_len;
        const int pol = (int)((e - row * row_len) / nbls), k = (int)(e % nbls);
        const int a1 = ant1[k], a2 = ant2[k];
        cplx<T> o = {(T)0, (T)0};
        if (a1 != a2 && (!weights || weights[e] > (T)0)) {  // else flagged: the datum is not read
            const int p = tpol == 4 ? (pol & 1) : 0, q = tpol == 4 ? (pol >> 1) : 0;
            const double c = (double)(row / ntimes) - 0.5 * (double)(nfreqs - 1);
            double sn, cs;
            sincos(-c * (slopes[q * nant + a2] - slopes[p * nant + a1]), &sn, &cs);
            const double dr = (double)data[e].re, di = (double)data[e].im;
            o = {(T)(dr * cs - di * sn), (T)(dr * sn + di * cs)};
        }
        out[e] = o;
    }
}
// Queues the two kernels of stage 1 on `on`.  All device pointers; weights may be null.  z: (nfeed npairs, nfreqs) scratch.
template <typename T>
inline void launch_firstcal_delays(hipStream_t on, const cplx<T> *data, const T *weights, const int *ant1, const int *ant2,
                                   int nbls, const int *pair1, const int *pair2, int nfreqs, int ntimes, int tpol, int npairs, const cplx<double> *tw, int nd,
                                   cplx<double> *z, int *peak_bin, double *delay_bins, double *power, double *total, int *used) {
    const int nfeed = tpol == 4 ? 2 : 1, nrows = nfeed * npairs;
    hipLaunchKernelGGL(k_firstcal_products<T>, dim3((unsigned)cdiv(npairs, 256), (unsigned)std::min(nfeed * nfreqs, 65535)), dim3(256), 0, on, data,
                       weights, ant1, ant2, pair1, pair2, nfreqs, ntimes, nbls, tpol, npairs, z);
    const size_t lds = sizeof(cplx<double>) * 4 * (size_t)nfreqs;
    const int in_lds = lds <= GAIN_LDS_BYTES;
    hipLaunchKernelGGL(k_firstcal_delay, dim3((unsigned)cdiv(nrows, 4)), dim3(256), in_lds ? lds : 0, on, (const cplx<double> *)z, tw,
                       nrows, nfreqs, nd, in_lds, peak_bin, delay_bins, power, total, used);
}

// ---------------------------------------------------------------------------------------------
// Abscal (fv_abscal_slopes, fv_abscal_evaluate; DESIGN.md "Abscal"): what the redundant solve above leaves free, fitted to a
// model of the group visibilities.  A row is a (solve unit, feed): a unit is a frequency (per_time = 0, its rows the
// frequency's ntimes times) or a (frequency, time); feed p reads the parallel hand pol = 3 p of the (nfreqs, ntimes, tpol,
// ngroups) blocks U (complex128), M (T) and W (float64, null: ones).  X: the groups' baselines in in-plane coordinates,
// x1 and x2 of ngroups doubles each (x2 = 0 for a line, ndim = 1).  Per row the fit maximises over the slope Phi
//     Re S(Phi),   S = sum_g c_g exp(i Phi . X_g),   c_g = sum_t W conj(U) M,   and then   eta = Re S / N,  N = sum W |U|^2.
// k_abscal_products: one thread per (row, group), the group fastest so that the loads coalesce; the unit's times ascending,
// every term formed and added in fp64: c_g, N_g = sum_t W |U|^2, P_g = sum_t W |M|^2 and the count of used samples.  A sample
// is used when W > 0 and X_g != 0 (an auto-correlation's own group is never used); a flagged datum is not read.  bad[0]
// counts weights that are negative or not finite, bad[1] values of U and bad[2] values of M that are not finite at a used
// sample (int atomics).  k_abscal_search: Re S on the grid Phi = (j_1 h_1, j_2 h_2), j_i = i_i - (n_i - 1) / 2, i_i = 0 ..
// n_i - 1 (n_i odd), and its argmax.  The kernel's axes are (a, b) with the runs along b: (1, 2), or (2, 1) for a line,
// where n_2 = 1 -- the flat index i_a n_b + i_b is i_1 n_2 + i_2 either way.  A thread owns one run of ABSCAL_RUN = 8
// consecutive i_b at one i_a; a block's 256 runs are a tile, the grid is (tiles, rows).  The groups pass through LDS in
// chunks of ABSCAL_CHUNK = 512 -- c, x_a, x_b and the step factor exp(i h_b x_b) (built on the host in fp64), six doubles
// a group, 24 576 bytes <= GAIN_LDS_BYTES -- and every thread reads the same group at a time (a broadcast: no bank
// conflict).  Per (group, run): the phase Phi . X in fp64 and one sincos at the run's first point, w = c exp(i Phi . X), then
// ABSCAL_RUN - 1 rotations w <- w step; every thread adds the groups in ascending order for its own slopes.  The argmax:
// a thread keeps the first maximum it meets, every reduction (an __shfl_xor tree, the block's waves through LDS, and
// k_abscal_peak, one wave per row over the tiles' winners) takes the larger value and on a tie the lower flat index.
// k_abscal_refine: one wave per row.  abscal_six_sums -- f = Re S, its gradient g_i = -sum X_i Im(c e^{i Phi . X}) and its
// Hessian H_ij = -sum X_i X_j Re(c e^{i Phi . X}) at the continuous Phi, sincos in fp64, lane l adding the groups l, l + 64,
// ..., an __shfl_xor tree (every lane ends with the same bits).  `refine` rounds of Newton from the grid's peak: where H is
// negative definite the step -H^-1 g, else g / max |eig H| (0 where H = 0), either clipped to +-h_i per dimension; one more
// evaluation at the result gives Re S.  A row is used when N > 0, at least ndim + 1 groups have a used sample and Re S > 0;
// one that is not reports eta = 1, Phi = 0, the peak (0, 0) and Re S = 0.  X and the four rows' c are staged in LDS when
// they fit GAIN_LDS_BYTES (80 ngroups bytes: ngroups <= 409), which is why a wave without a row stays for the barrier.
// k_abscal_chi2: sum W |eta e^{-i Phi . X} U - M|^2 per (frequency, time) over the feeds and the used samples, formed
// explicitly at the returned parameters (the closed form P - (Re S)^2 / N cancels): one thread per (feed, group), the
// block's partial by row_tail, the row's by k_chi2_rows_reduce.  No floating-point atomics: the same input gives the same
// bits.
constexpr int ABSCAL_RUN = 8;
constexpr int ABSCAL_CHUNK = 512;
static_assert(sizeof(double) * 6 * ABSCAL_CHUNK <= GAIN_LDS_BYTES, "a chunk of the search fits the staging budget");
template <typename T>
__global__ void __launch_bounds__(256)
    k_abscal_products(const cplx<double> *__restrict__ uvis, const cplx<T> *__restrict__ model, const double *__restrict__ gw,
                      const double *__restrict__ x1, const double *__restrict__ x2, int nunits, int ntimes, int tpol, int ngroups,
                      int per_time, cplx<double> *__restrict__ c, double *__restrict__ ng, double *__restrict__ pg,
                      int *__restrict__ cnt, int *__restrict__ bad) {
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (g >= ngroups) return;
    const bool cross = x1[g] != 0.0 || x2[g] != 0.0;
    const int nfeed = tpol == 4 ? 2 : 1;
    int bad_w = 0, bad_u = 0, bad_m = 0;
    for (int row = (int)blockIdx.y; row < nunits * nfeed; row += (int)gridDim.y) {
        const int unit = row / nfeed, feed = row - unit * nfeed;
        const int64_t r0 = per_time ? unit : (int64_t)unit * ntimes, r1 = per_time ? r0 + 1 : r0 + ntimes;
        double cr = 0.0, ci = 0.0, sn = 0.0, sp = 0.0;
        int n = 0;
        for (int64_t r = r0; r < r1; ++r) {  // ascending time
            const int64_t at = (r * tpol + 3 * feed) * ngroups + g;
            const double w = gw ? gw[at] : 1.0;
            if (!(w >= 0.0) || !isfinite(w)) ++bad_w;
            if (!(w > 0.0) || !cross) continue;  // flagged: the data are not read
            const cplx<double> u = uvis[at], m = {(double)model[at].re, (double)model[at].im};
            if (!isfinite(u.re) || !isfinite(u.im)) ++bad_u;
            if (!isfinite(m.re) || !isfinite(m.im)) ++bad_m;
            cr += w * (u.re * m.re + u.im * m.im);
            ci += w * (u.re * m.im - u.im * m.re);
            sn += w * (u.re * u.re + u.im * u.im);
            sp += w * (m.re * m.re + m.im * m.im);
            ++n;
        }
        const int64_t o = (int64_t)row * ngroups + g;
        c[o] = {cr, ci};
        ng[o] = sn;
        pg[o] = sp;
        cnt[o] = n;
    }
    if (bad_w) atomicAdd(bad, bad_w);
    if (bad_u) atomicAdd(bad + 1, bad_u);
    if (bad_m) atomicAdd(bad + 2, bad_m);
}
// larger value, on a tie the lower flat index
__device__ __forceinline__ void abscal_take(double &best, int &idx, double ob, int oi) {
    if (ob > best || (ob == best && oi < idx)) {
        best = ob;
        idx = oi;
    }
}
// c: (nrows, ngroups); xa, xb, step: (ngroups); tile_val, tile_idx: (nrows, gridDim.x)
__global__ void __launch_bounds__(256)
    k_abscal_search(const cplx<double> *__restrict__ c, const double *__restrict__ xa, const double *__restrict__ xb,
                    const cplx<double> *__restrict__ step, int nrows, int ngroups, int na, int nb, double ha, double hb,
                    double *__restrict__ tile_val, int *__restrict__ tile_idx) {
    __shared__ double stage[6][ABSCAL_CHUNK];
    __shared__ double wave_val[4];
    __shared__ int wave_idx[4];
    const int nruns_b = (nb + ABSCAL_RUN - 1) / ABSCAL_RUN;
    const int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool has = run < (int64_t)na * nruns_b;
    const int ia = has ? (int)(run / nruns_b) : 0, ib0 = has ? (int)(run % nruns_b) * ABSCAL_RUN : 0;
    const double pa = (double)(ia - (na - 1) / 2) * ha, pb = (double)(ib0 - (nb - 1) / 2) * hb;
    for (int row = (int)blockIdx.y; row < nrows; row += (int)gridDim.y) {
        double acc[ABSCAL_RUN];
#pragma unroll
        for (int j = 0; j < ABSCAL_RUN; ++j) acc[j] = 0.0;
        for (int g0 = 0; g0 < ngroups; g0 += ABSCAL_CHUNK) {
            const int m = min(ABSCAL_CHUNK, ngroups - g0);
            __syncthreads();  // (the chunk before has been read)
            for (int i = (int)threadIdx.x; i < m; i += 256) {
                const cplx<double> cg = c[(int64_t)row * ngroups + g0 + i], sg = step[g0 + i];
                stage[0][i] = cg.re;
                stage[1][i] = cg.im;
                stage[2][i] = xa[g0 + i];
                stage[3][i] = xb[g0 + i];
                stage[4][i] = sg.re;
                stage[5][i] = sg.im;
            }
            __syncthreads();
            for (int i = 0; has && i < m; ++i) {  // ascending group
                double sn, cs;
                sincos(pa * stage[2][i] + pb * stage[3][i], &sn, &cs);
                const double cr = stage[0][i], ci = stage[1][i], sr = stage[4][i], si = stage[5][i];
                double wr = cr * cs - ci * sn, wi = cr * sn + ci * cs;
                acc[0] += wr;
#pragma unroll
                for (int j = 1; j < ABSCAL_RUN; ++j) {
                    const double t = wr * sr - wi * si;
                    wi = wr * si + wi * sr;
                    wr = t;
                    acc[j] += wr;
                }
            }
        }
        double best = -INFINITY;
        int idx = has ? ia * nb + ib0 : INT_MAX;
#pragma unroll
        for (int j = 0; j < ABSCAL_RUN; ++j)
            if (has && ib0 + j < nb && acc[j] > best) {  // the first maximum
                best = acc[j];
                idx = ia * nb + ib0 + j;
            }
        for (int off = 32; off > 0; off >>= 1) abscal_take(best, idx, __shfl_xor(best, off, 64), __shfl_xor(idx, off, 64));
        if ((threadIdx.x & 63) == 0) {
            wave_val[threadIdx.x >> 6] = best;
            wave_idx[threadIdx.x >> 6] = idx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) abscal_take(best, idx, wave_val[w], wave_idx[w]);
            tile_val[(int64_t)row * gridDim.x + blockIdx.x] = best;
            tile_idx[(int64_t)row * gridDim.x + blockIdx.x] = idx;
        }
        __syncthreads();
    }
}
// the row's winner among its tiles': one wave per row
__global__ void __launch_bounds__(256)
    k_abscal_peak(const double *__restrict__ tile_val, const int *__restrict__ tile_idx, int nrows, int ntiles, int *__restrict__ peak_idx) {
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (row >= nrows) return;  // (whole waves)
    double best = -INFINITY;
    int idx = INT_MAX;
    for (int t = lane; t < ntiles; t += 64) abscal_take(best, idx, tile_val[(int64_t)row * ntiles + t], tile_idx[(int64_t)row * ntiles + t]);
    for (int off = 32; off > 0; off >>= 1) abscal_take(best, idx, __shfl_xor(best, off, 64), __shfl_xor(idx, off, 64));
    if (lane == 0) peak_idx[row] = idx;
}
// f, g_1, g_2, H_11, H_12, H_22 of Re S at (p1, p2): the wave's lanes split the groups; every lane returns the same bits
__device__ inline void abscal_six_sums(const cplx<double> *__restrict__ c, const double *__restrict__ x1, const double *__restrict__ x2,
                                       int ngroups, int lane, double p1, double p2, double s[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = 0.0;
    for (int g = lane; g < ngroups; g += 64) {
        const cplx<double> cg = c[g];
        const double a = x1[g], b = x2[g];
        double sn, cs;
        sincos(p1 * a + p2 * b, &sn, &cs);
        const double re = cg.re * cs - cg.im * sn, im = cg.re * sn + cg.im * cs;
        s[0] += re;
        s[1] -= a * im;
        s[2] -= b * im;
        s[3] -= a * a * re;
        s[4] -= a * b * re;
        s[5] -= b * b * re;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
        for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_xor(s[j], off, 64);
}
// The block's four rows as abscal_six_sums reads them: X and the rows' c staged in dynamic LDS when in_lds (5 ngroups
// complex128), else where they lie.  Every thread of the block calls it (a barrier); row: this wave's, clamped.
__device__ inline void abscal_stage(const cplx<double> *__restrict__ &c, const double *__restrict__ &x1, const double *__restrict__ &x2,
                                    int64_t row, int ngroups, int in_lds) {
    extern __shared__ __align__(16) unsigned char gain_lds[];
    c += row * ngroups;
    if (!in_lds) return;
    double *l1 = reinterpret_cast<double *>(gain_lds), *l2 = l1 + ngroups;
    cplx<double> *lc = reinterpret_cast<cplx<double> *>(l2 + ngroups) + (threadIdx.x >> 6) * ngroups;
    for (int g = (int)threadIdx.x; g < ngroups; g += 256) {
        l1[g] = x1[g];
        l2[g] = x2[g];
    }
    for (int g = (int)(threadIdx.x & 63); g < ngroups; g += 64) lc[g] = c[g];
    __syncthreads();
    c = lc;
    x1 = l1;
    x2 = l2;
}
// slopes: (nrows, 2); out: (nrows, 6)
__global__ void __launch_bounds__(256)
    k_abscal_evaluate(const cplx<double> *__restrict__ c, const double *__restrict__ x1, const double *__restrict__ x2,
                      const double *__restrict__ slopes, int nrows, int ngroups, int in_lds, double *__restrict__ out) {
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const bool active = row < nrows;
    abscal_stage(c, x1, x2, active ? row : 0, ngroups, in_lds);
    if (!active) return;  // (no barrier follows)
    double s[6];
    abscal_six_sums(c, x1, x2, ngroups, lane, slopes[2 * row], slopes[2 * row + 1], s);
    if (lane < 6) out[6 * (int64_t)row + lane] = s[lane];
}
// peak_idx: (nrows) flat grid indices i_1 n_2 + i_2; the outputs: (nrows), peak and slopes (nrows, 2)
__global__ void __launch_bounds__(256)
    k_abscal_refine(const cplx<double> *__restrict__ c, const double *__restrict__ x1, const double *__restrict__ x2,
                    const double *__restrict__ ng, const double *__restrict__ pg, const int *__restrict__ cnt,
                    const int *__restrict__ peak_idx, int nrows, int ngroups, int ndim, int n1, int n2, double h1, double h2, int refine,
                    int in_lds, int *__restrict__ peak, double *__restrict__ slopes, double *__restrict__ amp, double *__restrict__ power,
                    double *__restrict__ unorm, double *__restrict__ mnorm, int *__restrict__ used) {
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const bool active = row < nrows;
    abscal_stage(c, x1, x2, active ? row : 0, ngroups, in_lds);
    if (!active) return;  // (no barrier follows)
    double N = 0.0, P = 0.0;
    int groups_used = 0;
    for (int g = lane; g < ngroups; g += 64) {
        const int64_t o = (int64_t)row * ngroups + g;
        N += ng[o];
        P += pg[o];
        groups_used += cnt[o] > 0 ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        N += __shfl_xor(N, off, 64);
        P += __shfl_xor(P, off, 64);
        groups_used += __shfl_xor(groups_used, off, 64);
    }
    const int j1 = peak_idx[row] / n2 - (n1 - 1) / 2, j2 = peak_idx[row] % n2 - (n2 - 1) / 2;
    double p1 = (double)j1 * h1, p2 = ndim == 2 ? (double)j2 * h2 : 0.0, s[6];
    for (int round = 0; round < refine; ++round) {
        abscal_six_sums(c, x1, x2, ngroups, lane, p1, p2, s);
        double d1, d2 = 0.0;
        if (ndim == 1) {
            d1 = s[3] < 0.0 ? -s[1] / s[3] : (s[3] > 0.0 ? s[1] / s[3] : 0.0);
        } else {
            const double det = s[3] * s[5] - s[4] * s[4];
            if (s[3] < 0.0 && det > 0.0) {
                d1 = -(s[5] * s[1] - s[4] * s[2]) / det;
                d2 = -(s[3] * s[2] - s[4] * s[1]) / det;
            } else {
                const double hd = 0.5 * (s[3] - s[5]), big = fabs(0.5 * (s[3] + s[5])) + sqrt(hd * hd + s[4] * s[4]);
                d1 = big > 0.0 ? s[1] / big : 0.0;
                d2 = big > 0.0 ? s[2] / big : 0.0;
            }
        }
        p1 += fmin(fmax(d1, -h1), h1);
        if (ndim == 2) p2 += fmin(fmax(d2, -h2), h2);
    }
    abscal_six_sums(c, x1, x2, ngroups, lane, p1, p2, s);
    if (lane == 0) {
        const bool ok = N > 0.0 && groups_used >= ndim + 1 && s[0] > 0.0;
        peak[2 * row] = ok ? j1 : 0;
        peak[2 * row + 1] = ok ? j2 : 0;
        slopes[2 * row] = ok ? p1 : 0.0;
        slopes[2 * row + 1] = ok ? p2 : 0.0;
        amp[row] = ok ? s[0] / N : 1.0;
        power[row] = ok ? s[0] : 0.0;
        unorm[row] = N;
        mnorm[row] = P;
        used[row] = ok ? 1 : 0;
    }
}
// amp: (nunits nfeed), slopes: (nunits nfeed, 2); partials: (nfreqs ntimes, gridDim.x)
template <typename T>
__global__ void __launch_bounds__(256)
    k_abscal_chi2(const cplx<double> *__restrict__ uvis, const cplx<T> *__restrict__ model, const double *__restrict__ gw,
                  const double *__restrict__ x1, const double *__restrict__ x2, const double *__restrict__ amp,
                  const double *__restrict__ slopes, int64_t nrows, int ntimes, int tpol, int ngroups, int per_time,
                  double *__restrict__ partials) {
    const int nfeed = tpol == 4 ? 2 : 1;
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;  // (feed, group)
    const int feed = e / ngroups, g = e - feed * ngroups;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        double term = 0.0;
        if (feed < nfeed && (x1[g] != 0.0 || x2[g] != 0.0)) {
            const int64_t at = (row * tpol + 3 * feed) * ngroups + g, ur = (per_time ? row : row / ntimes) * nfeed + feed;
            const double w = gw ? gw[at] : 1.0;
            if (w > 0.0) {  // else flagged: the data are not read
                double sn, cs;
                sincos(slopes[2 * ur] * x1[g] + slopes[2 * ur + 1] * x2[g], &sn, &cs);
                const cplx<double> u = uvis[at];
                const double dr = amp[ur] * (u.re * cs + u.im * sn) - (double)model[at].re;
                const double di = amp[ur] * (u.im * cs - u.re * sn) - (double)model[at].im;
                term = w * __builtin_fma(dr, dr, di * di);
            }
        }
        row_tail(term, 0, 0, row, partials, nullptr);
    }
}
// What the entry points hold on the device for the groups: x1, x2 and, for the search, its axes (a, b) and step factors
struct AbscalGrid {
    const double *x1, *x2, *xa, *xb;
    const cplx<double> *step;
    int ndim, n1, n2, na, nb;
    double h1, h2, ha, hb;
};
inline int abscal_in_lds(int ngroups) { return sizeof(double) * 10 * (size_t)ngroups <= GAIN_LDS_BYTES; }
inline int64_t abscal_tiles(const AbscalGrid &ag) { return cdiv((int64_t)ag.na * cdiv(ag.nb, ABSCAL_RUN), 256); }
// Queues products, search, peak and refine on `on`.  All device pointers; gw may be null.  c: (nrows, ngroups), ng, pg, cnt
// alike, tile_val, tile_idx: (nrows, abscal_tiles), peak_idx: (nrows), bad: three zeroed counters; nrows = nunits nfeed.
template <typename T>
inline void launch_abscal_fit(hipStream_t on, const cplx<double> *uvis, const cplx<T> *model, const double *gw, const AbscalGrid &ag,
                              int nunits, int ntimes, int tpol, int ngroups, int per_time, int refine, cplx<double> *c, double *ng,
                              double *pg, int *cnt, int *bad, double *tile_val, int *tile_idx, int *peak_idx, int *peak, double *slopes,
                              double *amp, double *power, double *unorm, double *mnorm, int *used) {
    const int nrows = nunits * (tpol == 4 ? 2 : 1), ntiles = (int)abscal_tiles(ag), in_lds = abscal_in_lds(ngroups);
    const size_t lds = in_lds ? sizeof(double) * 10 * (size_t)ngroups : 0;
    hipLaunchKernelGGL(k_abscal_products<T>, dim3((unsigned)cdiv(ngroups, 256), (unsigned)std::min(nrows, 65535)), dim3(256), 0, on, uvis,
                       model, gw, ag.x1, ag.x2, nunits, ntimes, tpol, ngroups, per_time, c, ng, pg, cnt, bad);
    hipLaunchKernelGGL(k_abscal_search, dim3((unsigned)ntiles, (unsigned)std::min(nrows, 65535)), dim3(256), 0, on, (const cplx<double> *)c,
                       ag.xa, ag.xb, ag.step, nrows, ngroups, ag.na, ag.nb, ag.ha, ag.hb, tile_val, tile_idx);
    hipLaunchKernelGGL(k_abscal_peak, dim3((unsigned)cdiv(nrows, 4)), dim3(256), 0, on, (const double *)tile_val, (const int *)tile_idx,
                       nrows, ntiles, peak_idx);
    hipLaunchKernelGGL(k_abscal_refine, dim3((unsigned)cdiv(nrows, 4)), dim3(256), lds, on, (const cplx<double> *)c, ag.x1, ag.x2,
                       (const double *)ng, (const double *)pg, (const int *)cnt, (const int *)peak_idx, nrows, ngroups, ag.ndim, ag.n1,
                       ag.n2, ag.h1, ag.h2, refine, in_lds, peak, slopes, amp, power, unorm, mnorm, used);
}

// ---------------------------------------------------------------------------------------------
// Jones solve on a resident model (fv_jones_normal_rows, fv_jones_solve; DESIGN.md "Jones solve"): the gain solve above
// with one 2 x 2 matrix per antenna.  The block, the pairs and the incidence lists are the Jones kernels', tpol = 4; V, d
// and w are read only; a sample is used when w > 0 and a1 != a2.  The iterate is complex128 whatever T is, (nunits, 2, 2,
// nant) in the Jones layout J[(2 i + j) nant + a] = Gamma_a[i, j]; row `row` reads unit row / rows_per_unit.  For fixed V
// the least-squares problem in one antenna's matrix, the others held, is linear and splits into one 2 x 2 Hermitian system
// per measured feed (column) c of Gamma_a:
//     side 1 (a = a2, c = x), Z[x', y] = sum_{y'} V[x', y'] conj(G1[y', y]):  u[i] = conj(Z[i, y]),  t = d[x, y],
//     side 0 (a = a1, c = y), Y[x, y'] = sum_{x'} G2[x', x] V[x', y']:        u[i] = Y[x, i],        t = conj(d[x, y]),
//     A[i, j] += w[x, y] u[i] conj(u[j]),   b[i] += w[x, y] u[i] t      over the column's used samples,
// and with autos flagged gjones[:, c, a] = 2 (A Gamma_a[:, c] - b).  Both sides are one formula in the OTHER antenna's
// matrix Go: u_o[i] = Go[0, o] X[0, i] + Go[1, o] X[1, i], o the other antenna's measured feed, with X = V on side 0 and
// X = V^H on side 1.  So a lane reads the planes of V transposed and conjugated on side 1, those of d and w transposed
// on side 0 (d conjugated there), and from then on every lane runs the same code on sample (c, o) -- no index into a
// register array depends on the side.  k_jones_normal is k_jones_gradient's gather: one wave per (row, antenna), lane l
// takes the entries l, l + 64, ... in order, a baseline's four V, its used d and its w read once for both columns, every
// term formed and added in fp64 (16 accumulators: per column A00, A11, Re A01, Im A01, b[0], b[1]), an __shfl_xor tree,
// one store per value and wave.  The row's matrices are staged in LDS when they fit GAIN_LDS_BYTES; a wave without an
// antenna stays for the barriers.  CHI2 = true writes instead the wave's sum of w |V' - d|^2 over its side-0 entries --
// every baseline once -- into part[row nant + a], for k_gain_chi2_rows.  k_jones_update, one block per unit: the sums of
// the unit's rows in ascending order; a column is solved when A00 > 0, A11 > 0 and det = A00 A11 - |A01|^2 >
// 2^-30 A00 A11 (else both of its entries keep their values), Gamma^[:, c] = A^-1 b in closed form, Gamma <- Gamma^ on
// odd iterations and (Gamma^ + Gamma) / 2 on even ones, written into the OTHER buffer, and change[unit] =
// max |new - old| / max |new| over the 4 nant entries.  No floating-point atomics anywhere.
// A_out[((row 4 + q) 2 + c) nant + a], q = A00, A11, Re A01, Im A01;  b_out[((row 2 + i) 2 + c) nant + a].
template <typename T, bool CHI2>
__global__ void __launch_bounds__(256)
    k_jones_normal(const cplx<T> *__restrict__ vis, const cplx<T> *__restrict__ data, const T *__restrict__ weights,
                   const cplx<double> *__restrict__ jones, const int *__restrict__ ant1, const int *__restrict__ ant2,
                   const int *__restrict__ inc_off, const int *__restrict__ inc, int64_t nrows, int64_t rows_per_unit, int nbls,
                   int nant, int in_lds, double *__restrict__ A_out, cplx<double> *__restrict__ b_out) {
    extern __shared__ __align__(16) unsigned char gain_lds[];
    const int nj = 4 * nant;
    const int ant_w = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const bool active = ant_w < nant;  // (whole waves: the tree below stays inside one)
    const int ant = active ? ant_w : 0;
    const int i0 = active ? inc_off[ant] : 0, i1 = active ? inc_off[ant + 1] : 0;
    const int64_t L = 4 * (int64_t)nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<double> *J = jones + (row / rows_per_unit) * nj;
        if (in_lds) {
            cplx<double> *jl = reinterpret_cast<cplx<double> *>(gain_lds);
            for (int i = threadIdx.x; i < nj; i += 256) jl[i] = J[i];
            J = jl;
            __syncthreads();
        }
        double acc[2][8];  // per column: A00, A11, Re A01, Im A01, b[0], b[1]  (CHI2: acc[0][0] alone)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[c][q] = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            if (a1 == a2 || (CHI2 && side)) continue;  // an auto-correlation is flagged; chi2 counts a baseline once
            const int64_t e = row * L + k;
            // sample (c, o) = (this antenna's measured feed, the other's) lies in plane 2 x + y: 2 c + o on side 1, 2 o + c
            // on side 0; X[k', i] = V[k', i] (plane 2 k' + i) on side 0 and conj(V[i, k']) (plane 2 i + k') on side 1
            const int64_t ps = (int64_t)(side ? 1 : 2) * nbls, pt = (int64_t)(side ? 2 : 1) * nbls;
            const int64_t plane_s[4] = {0, ps, pt, 3 * (int64_t)nbls};  // of sample 2 c + o
            const int64_t plane_x[4] = {0, pt, ps, 3 * (int64_t)nbls};  // of X[k', i] at 2 k' + i
            double w[4];
            bool any = false;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const T wt = weights ? weights[e + plane_s[s]] : (T)1;
                w[s] = wt > (T)0 ? (double)wt : 0.0;
                any = any || wt > (T)0;
            }
            if (!any) continue;  // every sample flagged: nothing is added, V is not read
            const int other = side ? a1 : a2;
            const double sx = side ? -1.0 : 1.0;  // X = V^H on side 1;  t = conj(d) on side 0
            cplx<double> x[4], go[4], u[4];       // u_o[i] at [2 o + i]
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                x[p] = {(double)vis[e + plane_x[p]].re, sx * (double)vis[e + plane_x[p]].im};
                go[p] = J[p * nant + other];
            }
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int n = 0; n < 2; ++n) u[2 * o + n] = cadd(cmul(go[o], x[n]), cmul(go[2 + o], x[2 + n]));
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const int s = 2 * c + o;
                    if (!(w[s] > 0.0)) continue;  // (a flagged datum is not read)
                    const cplx<double> t = {(double)data[e + plane_s[s]].re, -sx * (double)data[e + plane_s[s]].im};
                    const cplx<double> u0 = u[2 * o], u1 = u[2 * o + 1];
                    if (CHI2) {  // side 0: conj(V'[x = o, y = c]) = sum_i conj(u_o[i]) Gamma_a[i, c], and t = conj(d)
                        const cplx<double> vp = cadd(cmul(cconj(u0), J[c * nant + ant]), cmul(cconj(u1), J[(2 + c) * nant + ant]));
                        const double dr = vp.re - t.re, di = vp.im - t.im;
                        acc[0][0] += w[s] * (dr * dr + di * di);
                    } else {
                        const cplx<double> a01 = cmul(u0, cconj(u1)), b0 = cmul(u0, t), b1 = cmul(u1, t);
                        acc[c][0] += w[s] * (u0.re * u0.re + u0.im * u0.im);
                        acc[c][1] += w[s] * (u1.re * u1.re + u1.im * u1.im);
                        acc[c][2] += w[s] * a01.re;
                        acc[c][3] += w[s] * a01.im;
                        acc[c][4] += w[s] * b0.re;
                        acc[c][5] += w[s] * b0.im;
                        acc[c][6] += w[s] * b1.re;
                        acc[c][7] += w[s] * b1.im;
                    }
                }
        }
        if (CHI2) {
            for (int off = 32; off > 0; off >>= 1) acc[0][0] += __shfl_xor(acc[0][0], off, 64);
            if (active && lane == 0) A_out[row * nant + ant] = acc[0][0];
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    for (int off = 32; off > 0; off >>= 1) acc[c][q] += __shfl_xor(acc[c][q], off, 64);
                if (active && lane == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) A_out[((row * 4 + q) * 2 + c) * nant + ant] = acc[c][q];
                    b_out[((row * 2 + 0) * 2 + c) * nant + ant] = {acc[c][4], acc[c][5]};
                    b_out[((row * 2 + 1) * 2 + c) * nant + ant] = {acc[c][6], acc[c][7]};
                }
            }
        }
        if (in_lds) __syncthreads();  // (the next row of this block stages its matrices again)
    }
}
// One block per solve unit; see above.  A, b: k_jones_normal's, (nunits rows_per_unit, ...); j_old, j_new: (nunits, 4 nant),
// two buffers; odd: the iteration's parity; solved[(unit 2 + c) nant + a].  A thread takes a (column, antenna).
__global__ void __launch_bounds__(256)
    k_jones_update(const double *__restrict__ A, const cplx<double> *__restrict__ b, const cplx<double> *__restrict__ j_old,
                   cplx<double> *__restrict__ j_new, int64_t rows_per_unit, int nant, int odd, double *__restrict__ change,
                   int *__restrict__ solved) {
    __shared__ double wave_max[2][4];
    const int64_t unit = blockIdx.x;
    double md = 0.0, mn = 0.0;  // max |new - old|^2, max |new|^2 (the square root is monotone: taken once, at the end)
    for (int i = threadIdx.x; i < 2 * nant; i += 256) {
        const int c = i / nant, a = i - c * nant;
        double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // A00, A11, Re A01, Im A01, b[0], b[1]
        for (int64_t r = 0; r < rows_per_unit; ++r) {  // ascending time
            const int64_t row = unit * rows_per_unit + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += A[((row * 4 + q) * 2 + c) * nant + a];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                s[4 + 2 * n] += b[((row * 2 + n) * 2 + c) * nant + a].re;
                s[5 + 2 * n] += b[((row * 2 + n) * 2 + c) * nant + a].im;
            }
        }
        const int64_t at0 = unit * 4 * nant + (int64_t)c * nant + a, at1 = at0 + 2 * (int64_t)nant;  // Gamma_a[0, c], [1, c]
        const cplx<double> g0 = j_old[at0], g1 = j_old[at1];
        cplx<double> n0 = g0, n1 = g1;
        const double det = s[0] * s[1] - (s[2] * s[2] + s[3] * s[3]);
        const bool ok = s[0] > 0.0 && s[1] > 0.0 && det > 0x1p-30 * (s[0] * s[1]);
        if (ok) {  // A^-1 = [[A11, -A01], [-conj(A01), A00]] / det
            const cplx<double> a01 = {s[2], s[3]}, b0 = {s[4], s[5]}, b1 = {s[6], s[7]};
            const cplx<double> m0 = cmul(a01, b1), m1 = cmul(cconj(a01), b0);
            n0 = {(s[1] * b0.re - m0.re) / det, (s[1] * b0.im - m0.im) / det};
            n1 = {(s[0] * b1.re - m1.re) / det, (s[0] * b1.im - m1.im) / det};
            if (!odd) {
                n0 = {0.5 * (n0.re + g0.re), 0.5 * (n0.im + g0.im)};
                n1 = {0.5 * (n1.re + g1.re), 0.5 * (n1.im + g1.im)};
            }
        }
        j_new[at0] = n0;
        j_new[at1] = n1;
        solved[(unit * 2 + c) * nant + a] = ok ? 1 : 0;
        const double d0r = n0.re - g0.re, d0i = n0.im - g0.im, d1r = n1.re - g1.re, d1i = n1.im - g1.im;
        md = fmax(md, fmax(d0r * d0r + d0i * d0i, d1r * d1r + d1i * d1i));
        mn = fmax(mn, fmax(n0.re * n0.re + n0.im * n0.im, n1.re * n1.re + n1.im * n1.im));
    }
    for (int off = 32; off > 0; off >>= 1) {
        md = fmax(md, __shfl_xor(md, off, 64));
        mn = fmax(mn, __shfl_xor(mn, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        wave_max[0][threadIdx.x >> 6] = md;
        wave_max[1][threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        md = fmax(fmax(wave_max[0][0], wave_max[0][1]), fmax(wave_max[0][2], wave_max[0][3]));
        mn = fmax(fmax(wave_max[1][0], wave_max[1][1]), fmax(wave_max[1][2], wave_max[1][3]));
        change[unit] = mn > 0.0 ? sqrt(md) / sqrt(mn) : 0.0;
    }
}
// Queues one evaluation of the 2 x 2 normal systems (A, b) or, with chi2_part (nrows, nant), of the chi2 partials on `on`.
// All device pointers; weights may be null.
template <typename T>
inline void launch_jones_normal(hipStream_t on, const cplx<T> *vis, const cplx<T> *data, const T *weights, const cplx<double> *jones,
                                const GainPairs &gp, int64_t nrows, int64_t rows_per_unit, double *A, cplx<double> *b,
                                double *chi2_part) {
    const int nbls = (int)gp.nbls, nant = gp.nant;
    const size_t lds = sizeof(cplx<double>) * 4 * (size_t)nant;
    const int in_lds = lds <= GAIN_LDS_BYTES;
    const dim3 grid((unsigned)cdiv(nant, 4), (unsigned)std::min<int64_t>(nrows, 65535));
    if (chi2_part)
        hipLaunchKernelGGL((k_jones_normal<T, true>), grid, dim3(256), in_lds ? lds : 0, on, vis, data, weights, jones,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, nant, in_lds, chi2_part, (cplx<double> *)nullptr);
    else
        hipLaunchKernelGGL((k_jones_normal<T, false>), grid, dim3(256), in_lds ? lds : 0, on, vis, data, weights, jones,
                           gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), gp.d_off.as<int>(), gp.d_inc.as<int>(), nrows, rows_per_unit,
                           nbls, nant, in_lds, A, b);
}

// ---------------------------------------------------------------------------------------------
// The gain gradient of the Gauss-Newton product with gains (fv_gain_weight_rows, fv_sim_gain_weight_block; DESIGN.md
// "Gains in the Gauss-Newton product").  The block, the pairs, the feeds and the gains' layout are the gain kernels'
// above; dg is the gain direction in the gains' layout, or null.  With g1, g2, h1, h2, m, dm, U' and G' of
// k_weight_rows<T, NP, true>,
//     hgains[a, f] = sum_{k: a1 = a, p = f} conj(G') g2 V + sum_{k: a2 = a, q = f} G' g1 conj(V).
// k_gain_weight_gather is k_gain_gradient with this G' in place of 2 w (V' - d): it runs first, while the blocks still
// hold the parts and V, one wave per (row, feed, antenna) over the incidence lists, everything in fp64 from the T-typed
// inputs (U summed in fp64 in the parts' order), an __shfl_xor tree, one complex128 per wave; a flagged sample is skipped
// before its parts and V are read.  k_weight_rows<T, NP, true> follows.
// hgains[(row nfeed + feed) nant + a]: one wave per (row, feed, antenna); see above.  The parts and vis still hold the
// tangent parts and V.
template <typename T, int NP>
__global__ void __launch_bounds__(256)
    k_gain_weight_gather(WeightParts<T> parts, const cplx<T> *__restrict__ vis, const T *__restrict__ weights,
                         const cplx<T> *__restrict__ gains, const cplx<T> *__restrict__ dgains, const int *__restrict__ ant1,
                         const int *__restrict__ ant2, const int *__restrict__ inc_off, const int *__restrict__ inc,
                         int64_t nrows, int nbls, int tpol, int nant, cplx<double> *__restrict__ hgains) {
    const int nfeed = tpol == 4 ? 2 : 1, ng = nfeed * nant;
    const int wave = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (wave >= ng) return;  // (whole waves: the tree below stays inside one)
    const int feed = wave / nant, ant = wave - feed * nant;
    const int i0 = inc_off[ant], i1 = inc_off[ant + 1];
    const int64_t L = (int64_t)tpol * nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *g = gains + row * ng;
        const cplx<T> *h = dgains ? dgains + row * ng : nullptr;
        double sr = 0.0, si = 0.0;
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            for (int o = 0; o < nfeed; ++o) {  // the other antenna's feed
                const int p = side ? o : feed, q = side ? feed : o;
                const int64_t e = row * L + (int64_t)(nfeed == 2 ? 2 * q + p : 0) * nbls + k;
                const T wt = weights ? weights[e] : (T)1;
                if (!(wt > (T)0)) continue;  // flagged: nothing is added, the parts and V are not read
                const cplx<double> g1 = {(double)g[p * nant + a1].re, (double)g[p * nant + a1].im};
                const cplx<double> g2 = {(double)g[q * nant + a2].re, (double)g[q * nant + a2].im};
                const cplx<double> v = {(double)vis[e].re, (double)vis[e].im};
                const cplx<double> m = cmul(cconj(g1), g2);
                cplx<double> up = {0.0, 0.0};  // U' = m U + dm V
                if (NP) {
                    cplx<double> u = {(double)parts.p[0][e].re, (double)parts.p[0][e].im};
#pragma unroll
                    for (int n = 1; n < NP; ++n) u = {u.re + (double)parts.p[n][e].re, u.im + (double)parts.p[n][e].im};
                    up = cmul(m, u);
                }
                if (h) {
                    const cplx<double> h1 = {(double)h[p * nant + a1].re, (double)h[p * nant + a1].im};
                    const cplx<double> h2 = {(double)h[q * nant + a2].re, (double)h[q * nant + a2].im};
                    const cplx<double> m1 = cmul(cconj(h1), g2), m2 = cmul(cconj(g1), h2);
                    const cplx<double> t = cmul(cplx<double>{m1.re + m2.re, m1.im + m2.im}, v);
                    up = {up.re + t.re, up.im + t.im};
                }
                const double w2 = 2.0 * (double)wt;
                const cplx<double> gp = {w2 * up.re, w2 * up.im};
                // side 0: conj(G') g2 V;  side 1: G' g1 conj(V)
                const cplx<double> t = side ? cmul(gp, cmul(g1, cconj(v))) : cmul(cconj(gp), cmul(g2, v));
                sr += t.re;
                si += t.im;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off, 64);
            si += __shfl_xor(si, off, 64);
        }
        if (lane == 0) hgains[(row * nfeed + feed) * nant + ant] = {sr, si};
    }
}
// ---------------------------------------------------------------------------------------------
// Gauss-Newton product with Jones gains (fv_jones_weight_rows, fv_sim_jones_weight_block; DESIGN.md "Jones matrices in the
// Gauss-Newton product"): the product of the Jones objective's chi2 along a joint direction (sky directions, dGamma).  The
// block, the pairs, the incidence lists and the matrices' layout are the Jones kernels' above, tpol = 4; H1 = dGamma[a1],
// H2 = dGamma[a2] are the direction's matrices in the same layout (or none), U the sum of the NP tangent parts (0 for NP = 0,
// the matrices-only direction), V the forward at the real parameters.  With S(X; A, B)[x, y] = sum_{x', y'} conj(A[y', y])
// B[x', x] X[x', y'] the data model's product (V' = S(V; G1, G2)),
//     U' = S(U; G1, G2) + S(V; H1, G2) + S(V; G1, H2)   (the first term alone without a direction, the last two for NP = 0),
//     G'[x, y] = 2 (w[x, y] U'[x, y]),   row sum += w |U'|^2,   stored G = the Jones objective's G of this G' (jones_stored_g),
//     hjones = gjones' two sums with this G' (M = G2^T V on side 0, V conj G1 on side 1).
// Flags are the Jones objective's: w == 0 flags that one (x, y) sample -- G' = 0 exactly there, nothing is added to the rows
// or to hjones, the baseline's other samples still use all four values of U and V --, and a baseline with all four samples
// flagged stores G = 0 exactly whatever its parts and V hold.  V is read only with a direction; G replaces P_0, or V for
// NP = 0.  Two kernels, no floating-point atomics.  k_jones_weight_gather runs first, while the blocks still hold the parts
// and V; k_jones_weight_rows follows, in place, with k_jones_residual_rows' thread-to-baseline mapping; its row terms go to
// `terms` and k_jones_rows_sum and k_chi2_rows_reduce add them.  In T every operation rounds on its own (no contraction), in
// this order, every sum of two products left to right and the products as jones_mul / jones_mulc write them:
//     U = ((P_0 + P_1) + P_2) + P_3 (component-wise, only the parts given),
//     S(X; A, B):  B'[x', y] = X[x', 0] conj(A[0, y]) + X[x', 1] conj(A[1, y]),   S[x, y] = B[0, x] B'[0, y] + B[1, x] B'[1, y]
//     (jones_residual_baseline's V'),   U' = (S(U; G1, G2) + S(V; H1, G2)) + S(V; G1, H2)  (component-wise),
//     G' = 2 (w U'),   then jones_stored_g.
// With identity matrices and no direction S(U) = U and G = G' exactly: k_weight_rows<T, NP, false>'s bits, rows included.
template <typename T>
__device__ __forceinline__ void jones_sandwich(const cplx<T> (&x)[4], const cplx<T> (&ga)[4], const cplx<T> (&gb)[4],
                                               cplx<T> (&s)[4]) {  // S(X; A, B), see above
#pragma clang fp contract(off)
    cplx<T> b[4];
#pragma unroll
    for (int xs = 0; xs < 2; ++xs)
#pragma unroll
        for (int y = 0; y < 2; ++y) b[2 * xs + y] = jones_add(jones_mulc(x[2 * xs], ga[y]), jones_mulc(x[2 * xs + 1], ga[2 + y]));
#pragma unroll
    for (int xx = 0; xx < 2; ++xx)
#pragma unroll
        for (int y = 0; y < 2; ++y) s[2 * xx + y] = jones_add(jones_mul(gb[xx], b[y]), jones_mul(gb[2 + xx], b[2 + y]));
}
// One baseline (a1, a2) in place: u[2 x + y] = U -> G (U is ignored when SKY is false), v = V (read only with H), the row
// terms of its four samples, the count of bad weights.  J, H: the row's matrices and direction (staged or global; H null: no
// direction), entry [2 i + j] of antenna a at [(2 i + j) nant + a].
template <typename T, bool SKY>
__device__ __forceinline__ void jones_weight_baseline(cplx<T> (&u)[4], const cplx<T> (&v)[4], const T (&w)[4], const cplx<T> *J,
                                                      const cplx<T> *H, int nant, int a1, int a2, double (&term)[4], int &bad_w) {
#pragma clang fp contract(off)
    const cplx<T> g1[4] = {J[a1], J[nant + a1], J[2 * nant + a1], J[3 * nant + a1]};
    const cplx<T> g2[4] = {J[a2], J[nant + a2], J[2 * nant + a2], J[3 * nant + a2]};
    cplx<T> up[4], gp[4];  // U'[x, y], G'[x, y] at [2 x + y]
    if constexpr (SKY) jones_sandwich<T>(u, g1, g2, up);
    if (H) {
        cplx<T> d[4];
        {
            const cplx<T> h1[4] = {H[a1], H[nant + a1], H[2 * nant + a1], H[3 * nant + a1]};
            jones_sandwich<T>(v, h1, g2, d);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) up[s] = SKY ? jones_add(up[s], d[s]) : d[s];
        {
            const cplx<T> h2[4] = {H[a2], H[nant + a2], H[2 * nant + a2], H[3 * nant + a2]};
            jones_sandwich<T>(v, g1, h2, d);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) up[s] = jones_add(up[s], d[s]);
    } else if constexpr (!SKY) {  // (the launcher refuses NP = 0 without a direction)
#pragma unroll
        for (int s = 0; s < 4; ++s) up[s] = {(T)0, (T)0};
    }
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (!(w[s] >= (T)0) || !isfinite(w[s])) ++bad_w;
        if (w[s] > (T)0) {
            gp[s] = {(T)2 * (w[s] * up[s].re), (T)2 * (w[s] * up[s].im)};
            term[s] = row_term<T>(w[s], up[s].re, up[s].im);
            any = true;
        } else {  // flagged (or counted above)
            gp[s] = {(T)0, (T)0};
            term[s] = 0.0;
        }
    }
    jones_stored_g<T>(gp, g1, g2, any, u);
}
// One baseline of a row: its four values at e, e + nbls, ... of the block's index.
template <typename T, int NP>
__device__ __forceinline__ void jones_weight_at(int64_t e, int nbls, int a1, int a2, const cplx<T> *J, const cplx<T> *H, int nant,
                                                const WeightParts<T> &parts, cplx<T> *vis, cplx<T> *out,
                                                const T *__restrict__ weights, double *__restrict__ terms, int &bad_w) {
#pragma clang fp contract(off)
    cplx<T> u[4], v[4];
    T w[4];
    double term[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t ep = e + (int64_t)p * nbls;
        u[p] = {(T)0, (T)0};
        if constexpr (NP > 0) u[p] = parts.p[0][ep];
#pragma unroll
        for (int n = 1; n < NP; ++n) u[p] = {u[p].re + parts.p[n][ep].re, u[p].im + parts.p[n][ep].im};
        v[p] = H ? vis[ep] : cplx<T>{(T)0, (T)0};
        w[p] = weights ? weights[ep] : (T)1;
    }
    jones_weight_baseline<T, (NP > 0)>(u, v, w, J, H, nant, a1, a2, term, bad_w);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        out[e + (int64_t)p * nbls] = u[p];
        terms[e + (int64_t)p * nbls] = term[p];
    }
}
// In place over (nrows, 4 nbls) blocks; see above.  lds_j: the row's matrices are staged in dynamic LDS; lds_h: the
// direction too, behind them (only with lds_j).  vec: every array is 16-byte aligned.
template <typename T, int NP>
__global__ void __launch_bounds__(256)
    k_jones_weight_rows(WeightParts<T> parts, cplx<T> *vis, const T *__restrict__ weights, const cplx<T> *__restrict__ jones,
                        const cplx<T> *__restrict__ djones, const int *__restrict__ ant1, const int *__restrict__ ant2,
                        int64_t nrows, int nbls, int nant, int lds_j, int lds_h, int vec, double *__restrict__ terms,
                        int *__restrict__ bad) {
    static_assert(NP >= 0 && NP <= 4, "NP = 0 .. 4");
    constexpr int W = RES_W<T>;
    constexpr int R = 16 / (int)sizeof(cplx<T>);  // the baselines of one 16-byte vector of a plane: 1 (fp64) or 2 (fp32)
    extern __shared__ __align__(16) unsigned char gain_lds[];
    const int nj = 4 * nant;
    const int64_t L = 4 * (int64_t)nbls;
    cplx<T> *const out = NP ? parts.p[0] : vis;  // where G goes
    const bool runs = R > 1 && vec && nbls % R == 0;  // (k_jones_residual_rows' runs)
    const int step = runs ? R : 1, nit = RES_CHUNKS * W / step;
    int bad_w = 0;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *J = jones + row * nj;
        const cplx<T> *H = djones ? djones + row * nj : nullptr;
        if (lds_j) {
            cplx<T> *jl = reinterpret_cast<cplx<T> *>(gain_lds);
            for (int i = threadIdx.x; i < nj; i += 256) jl[i] = J[i];
            J = jl;
            if (H && lds_h) {
                for (int i = threadIdx.x; i < nj; i += 256) jl[nj + i] = H[i];
                H = jl + nj;
            }
            __syncthreads();
        }
        const int64_t lo = row * L;
        const int shift = runs ? (int)(lo % R) : 0;  // run r holds the baselines [r R - shift, r R - shift + R)
        const int64_t kblock = (int64_t)blockIdx.x * (RES_CHUNKS * 256 * W) - shift;
        for (int i = 0; i < nit; ++i) {
            const int64_t k0 = kblock + ((int64_t)i * 256 + threadIdx.x) * step;
            if (k0 >= nbls) break;
            if constexpr (R > 1) {
                if (runs && k0 >= 0 && k0 + R <= nbls) {
                    union {
                        uint4 q;
                        cplx<T> c[R];
                    } u[4], v[4], t;
                    T w[4][R];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int64_t e = lo + (int64_t)p * nbls + k0;
                        if constexpr (NP > 0) u[p].q = *reinterpret_cast<const uint4 *>(parts.p[0] + e);
#pragma unroll
                        for (int n = 1; n < NP; ++n) {
                            t.q = *reinterpret_cast<const uint4 *>(parts.p[n] + e);
#pragma unroll
                            for (int j = 0; j < R; ++j) u[p].c[j] = {u[p].c[j].re + t.c[j].re, u[p].c[j].im + t.c[j].im};
                        }
                        if (H) v[p].q = *reinterpret_cast<const uint4 *>(vis + e);
#pragma unroll
                        for (int j = 0; j < R; ++j) w[p][j] = weights ? weights[e + j] : (T)1;
                    }
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        const cplx<T> zero = {(T)0, (T)0};
                        cplx<T> uu[4] = {zero, zero, zero, zero};
                        if constexpr (NP > 0) {
#pragma unroll
                            for (int p = 0; p < 4; ++p) uu[p] = u[p].c[j];
                        }
                        const cplx<T> vv[4] = {H ? v[0].c[j] : zero, H ? v[1].c[j] : zero, H ? v[2].c[j] : zero,
                                               H ? v[3].c[j] : zero};
                        const T w4[4] = {w[0][j], w[1][j], w[2][j], w[3][j]};
                        double term[4];
                        jones_weight_baseline<T, (NP > 0)>(uu, vv, w4, J, H, nant, ant1[k0 + j], ant2[k0 + j], term, bad_w);
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            u[p].c[j] = uu[p];
                            terms[lo + (int64_t)p * nbls + k0 + j] = term[p];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) *reinterpret_cast<uint4 *>(out + lo + (int64_t)p * nbls + k0) = u[p].q;
                    continue;
                }
            }
            const int64_t kb = k0 + step < nbls ? k0 + step : nbls;
            for (int64_t k = k0 > 0 ? k0 : 0; k < kb; ++k)
                jones_weight_at<T, NP>(lo + k, nbls, ant1[k], ant2[k], J, H, nant, parts, vis, out, weights, terms, bad_w);
        }
        if (lds_j) __syncthreads();  // (the next row of this block stages its matrices again)
    }
    if (bad_w) atomicAdd(bad, bad_w);
}
// hjones[((row 2 + i) 2 + j) nant + a]: k_jones_gradient with the G' above in place of 2 w (V' - d): one wave per (row,
// antenna) holds all four entries of the antenna's matrix, lane l takes the entries l, l + 64, ... of the incidence list in
// order, everything is formed in fp64 from the T-typed inputs (U summed in fp64 in the parts' order), an __shfl_xor tree,
// four complex128 per wave; a baseline whose four samples are all flagged is skipped before anything of it is read; an
// antenna without a baseline gets exactly 0.  The parts and vis still hold the tangent parts and V.
template <typename T, int NP>
__global__ void __launch_bounds__(256)
    k_jones_weight_gather(WeightParts<T> parts, const cplx<T> *__restrict__ vis, const T *__restrict__ weights,
                          const cplx<T> *__restrict__ jones, const cplx<T> *__restrict__ djones, const int *__restrict__ ant1,
                          const int *__restrict__ ant2, const int *__restrict__ inc_off, const int *__restrict__ inc,
                          int64_t nrows, int nbls, int nant, cplx<double> *__restrict__ hjones) {
    const int ant = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (ant >= nant) return;  // (whole waves: the tree below stays inside one)
    const int i0 = inc_off[ant], i1 = inc_off[ant + 1];
    const int64_t L = 4 * (int64_t)nbls;
    for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
        const cplx<T> *J = jones + row * 4 * nant;
        const cplx<T> *H = djones ? djones + row * 4 * nant : nullptr;
        cplx<double> acc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        for (int i = i0 + lane; i < i1; i += 64) {
            const int k = inc[i] >> 1, side = inc[i] & 1;
            const int a1 = ant1[k], a2 = ant2[k];
            const int64_t e = row * L + k;
            cplx<double> v[4], g1[4], g2[4], m[4], up[4], gp[4];
            double w2[4];
            bool any = false;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const T wt = weights ? weights[e + (int64_t)p * nbls] : (T)1;
                w2[p] = wt > (T)0 ? 2.0 * (double)wt : 0.0;
                any = any || wt > (T)0;
            }
            if (!any) continue;  // every sample flagged: nothing is added, nothing more is read
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                v[p] = {(double)vis[e + (int64_t)p * nbls].re, (double)vis[e + (int64_t)p * nbls].im};
                g1[p] = {(double)J[p * nant + a1].re, (double)J[p * nant + a1].im};
                g2[p] = {(double)J[p * nant + a2].re, (double)J[p * nant + a2].im};
                up[p] = {0.0, 0.0};
            }
            if constexpr (NP > 0) {
                cplx<double> u[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int64_t ep = e + (int64_t)p * nbls;
                    u[p] = {(double)parts.p[0][ep].re, (double)parts.p[0][ep].im};
#pragma unroll
                    for (int n = 1; n < NP; ++n) u[p] = {u[p].re + (double)parts.p[n][ep].re, u[p].im + (double)parts.p[n][ep].im};
                }
                jones_sandwich<double>(u, g1, g2, up);
            }
            if (H) {
                cplx<double> h[4], d[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) h[p] = {(double)H[p * nant + a1].re, (double)H[p * nant + a1].im};
                jones_sandwich<double>(v, h, g2, d);
#pragma unroll
                for (int p = 0; p < 4; ++p) up[p] = cadd(up[p], d[p]);
#pragma unroll
                for (int p = 0; p < 4; ++p) h[p] = {(double)H[p * nant + a2].re, (double)H[p * nant + a2].im};
                jones_sandwich<double>(v, g1, h, d);
#pragma unroll
                for (int p = 0; p < 4; ++p) up[p] = cadd(up[p], d[p]);
            }
            // side 0: M[x, y'] = (G2^T V)[x, y'] at [2 x + y'];  side 1: M[x', y] = (V conj G1)[x', y] at [2 x' + y]
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    m[2 * r + c] = side ? cadd(cmul(v[2 * r], cconj(g1[c])), cmul(v[2 * r + 1], cconj(g1[2 + c])))
                                        : cadd(cmul(g2[r], v[c]), cmul(g2[2 + r], v[2 + c]));
#pragma unroll
            for (int s = 0; s < 4; ++s)  // (a select: exactly 0 where flagged)
                gp[s] = w2[s] > 0.0 ? cplx<double>{w2[s] * up[s].re, w2[s] * up[s].im} : cplx<double>{0.0, 0.0};
            // side 0: acc[y', y] += sum_x conj(G'[x, y]) M[x, y'];  side 1: acc[x', x] += sum_y G'[x, y] conj(M[x', y])
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const cplx<double> t = side ? cadd(cmul(gp[2 * c], cconj(m[2 * r])), cmul(gp[2 * c + 1], cconj(m[2 * r + 1])))
                                                : cadd(cmul(cconj(gp[c]), m[r]), cmul(cconj(gp[2 + c]), m[2 + r]));
                    acc[2 * r + c].re += t.re;
                    acc[2 * r + c].im += t.im;
                }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            for (int off = 32; off > 0; off >>= 1) {
                acc[s].re += __shfl_xor(acc[s].re, off, 64);
                acc[s].im += __shfl_xor(acc[s].im, off, 64);
            }
            if (lane == 0) hjones[(row * 4 + s) * nant + ant] = acc[s];
        }
    }
}
// The calibration of a row pass, all device pointers: its kind, the pairs (None: no pairs, and nothing else is read), the
// rows' gains (nrows, nfeed nant) or matrices (nrows, 2, 2, nant) x and their direction dx (null: no direction, and none
// in the objective), where the gradient goes (the shape of x in complex128; null: the gather does not run) and, for
// Jones, the rows' terms (nrows, 4 nbls) fp64.
enum class Cal { None, Gains, Jones };
// entries of x per row
inline int cal_entries(Cal kind, int tpol, int nant) { return kind == Cal::Jones ? 4 * nant : kind == Cal::Gains ? (tpol == 4 ? 2 : 1) * nant : 0; }
template <typename T>
struct RowCal {
    Cal kind = Cal::None;
    const GainPairs *pairs = nullptr;
    const cplx<T> *x = nullptr, *dx = nullptr;
    cplx<double> *grad = nullptr;
    double *terms = nullptr;
};
// what the launchers share: vectors are allowed when every array's pointer is 16-byte aligned (null counts as aligned)
inline int rows_vec(std::initializer_list<const void *> arrays) {
    uintptr_t bits = 0;
    for (const void *a : arrays) bits |= reinterpret_cast<uintptr_t>(a);
    return (bits & 15) == 0;
}
// of a row pass with a calibration: the launch's numbers and the dynamic LDS of what it stages.  Gains and their direction
// are staged together or not at all; a row's matrices are staged when they fit GAIN_LDS_BYTES, the direction too when both
// fit together.  The Jones kernels walk chunks of baselines, so their grid has residual_blocks_per_row of nbls.
template <typename T>
struct RowCalShape {
    int nbls = 0, nant = 0, nfeed = 1, tpol = 1, nx = 0, lds_x = 0, lds_dx = 0;
    unsigned nblk_jones = 0;
    size_t shm = 0;
    const int *a1 = nullptr, *a2 = nullptr, *off = nullptr, *inc = nullptr;
    RowCalShape(const RowCal<T> &c, int64_t L) {
        if (c.kind == Cal::None) return;
        nbls = (int)c.pairs->nbls, nant = c.pairs->nant, tpol = (int)(L / nbls), nfeed = tpol == 4 ? 2 : 1;
        nx = cal_entries(c.kind, tpol, nant);
        a1 = c.pairs->d_ant1.template as<int>(), a2 = c.pairs->d_ant2.template as<int>();
        off = c.pairs->d_off.template as<int>(), inc = c.pairs->d_inc.template as<int>();
        const size_t one = sizeof(cplx<T>) * (size_t)nx, both = c.dx ? 2 * one : one;
        lds_x = (c.kind == Cal::Jones ? one : both) <= GAIN_LDS_BYTES;
        lds_dx = c.dx && both <= GAIN_LDS_BYTES;
        shm = lds_x ? (lds_dx ? both : one) : 0;
        nblk_jones = (unsigned)residual_blocks_per_row<T>(nbls);
    }
};
// f(std::integral_constant<int, nparts>) for nparts = 0 .. 4 (checked by the caller): the kernels take it at compile time
template <typename F>
inline void with_nparts(int nparts, F &&f) {
    switch (nparts) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}
// Queues the objective's kernels on `on`: the gather (k_gain_gradient or k_jones_gradient; with a calibration, when
// cal.grad is not null), the in-place kernel, for Jones the rows' sums of the terms, and the rows' reduction.  vis
// (nrows, L) in place, L = 4 nbls for Jones; rs from row_scratch for that shape (the counters are zeroed here).  All device
// pointers; weights may be null.
template <typename T>
inline void launch_residual(hipStream_t on, cplx<T> *vis, const cplx<T> *data, const T *weights, int64_t nrows, int64_t L,
                            const RowScratch &rs, const RowCal<T> &cal = {}) {
    const RowCalShape<T> cs(cal, L);
    const int vec = rows_vec({vis, data, weights});
    const unsigned rows_y = (unsigned)std::min<int64_t>(nrows, 65535);
    const dim3 grid((unsigned)rs.nblk, rows_y), gather((unsigned)cdiv(cal.kind == Cal::Jones ? cs.nant : cs.nx, 4), rows_y);
    FV_HIP(hipMemsetAsync(rs.bad, 0, 2 * sizeof(int), on));
    if (cal.kind == Cal::Jones) {
        if (cal.grad)
            hipLaunchKernelGGL(k_jones_gradient<T>, gather, dim3(256), 0, on, (const cplx<T> *)vis, data, weights, cal.x, cs.a1, cs.a2,
                               cs.off, cs.inc, nrows, cs.nbls, cs.nant, cal.grad);
        hipLaunchKernelGGL(k_jones_residual_rows<T>, dim3(cs.nblk_jones, rows_y), dim3(256), cs.shm, on, vis, data, weights, cal.x,
                           cs.a1, cs.a2, nrows, cs.nbls, cs.nant, cs.lds_x, vec, cal.terms, rs.bad);
        hipLaunchKernelGGL(k_jones_rows_sum<T>, grid, dim3(256), 0, on, (const double *)cal.terms, nrows, L, rs.partials, rs.bad);
    } else {
        if (cal.kind == Cal::Gains && cal.grad)
            hipLaunchKernelGGL(k_gain_gradient<T>, gather, dim3(256), 0, on, (const cplx<T> *)vis, data, weights, cal.x, cs.a1, cs.a2,
                               cs.off, cs.inc, nrows, cs.nbls, cs.tpol, cs.nant, cal.grad);
        const auto rows = [&](auto gains) {
            hipLaunchKernelGGL((k_residual_rows<T, decltype(gains)::value>), grid, dim3(256), cs.shm, on, vis, data, weights, cal.x,
                               cs.a1, cs.a2, nrows, L, cs.nbls, cs.nant, cs.nfeed, cs.lds_x, vec, rs.partials, rs.bad);
        };
        cal.kind == Cal::Gains ? rows(std::true_type{}) : rows(std::false_type{});
    }
    hipLaunchKernelGGL(k_chi2_rows_reduce, dim3((unsigned)cdiv(nrows, 256)), dim3(256), 0, on, (const double *)rs.partials, nrows,
                       rs.nblk, rs.sums);
}
// Queues the product's kernels on `on`: the gather (k_gain_weight_gather or k_jones_weight_gather; with a calibration,
// when cal.grad is not null), the in-place kernel, for Jones the rows' sums of the terms, and the rows' reduction.
// parts[0 .. nparts) device blocks (nrows, L), nparts = 1 .. 4, or 0 .. 4 with a calibration (0 needs cal.dx); vis the
// forward block (needed with cal.dx, with cal.grad and for nparts = 0; else it may be null); G in place in parts[0], or in
// vis for nparts = 0; rs from row_scratch for that shape (the counters are zeroed here).  weights may be null.
template <typename T>
inline void launch_weight_rows(hipStream_t on, int nparts, cplx<T> *const *parts, cplx<T> *vis, const T *weights, int64_t nrows,
                               int64_t L, const RowScratch &rs, const RowCal<T> &cal = {}) {
    const bool none = cal.kind == Cal::None, jones = cal.kind == Cal::Jones;
    if (none && (nparts < 1 || nparts > 4)) throw Error(FV_ERR_ARG, "nparts must be 1 .. 4");
    if (!none && (nparts < 0 || nparts > 4 || (nparts == 0 && !cal.dx)))
        throw Error(FV_ERR_ARG, jones ? "nparts must be 0 .. 4, and 0 needs d_jones" : "nparts must be 0 .. 4, and 0 needs d_gains");
    if (!none && (cal.dx || cal.grad || nparts == 0) && !vis)
        throw Error(FV_ERR_ARG, jones ? "d_jones and hjones need vis" : "d_gains and hgains need vis");
    const RowCalShape<T> cs(cal, L);
    WeightParts<T> wp{};
    for (int j = 0; j < nparts; ++j) wp.p[j] = parts[j];
    const int vec = rows_vec({weights, cal.dx || nparts == 0 ? vis : nullptr, wp.p[0], wp.p[1], wp.p[2], wp.p[3]});
    const unsigned rows_y = (unsigned)std::min<int64_t>(nrows, 65535);
    const dim3 grid((unsigned)rs.nblk, rows_y), gather((unsigned)cdiv(jones ? cs.nant : cs.nx, 4), rows_y);
    FV_HIP(hipMemsetAsync(rs.bad, 0, 2 * sizeof(int), on));
    with_nparts(nparts, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        if (jones) {
            if (cal.grad)
                hipLaunchKernelGGL((k_jones_weight_gather<T, NP>), gather, dim3(256), 0, on, wp, (const cplx<T> *)vis, weights, cal.x,
                                   cal.dx, cs.a1, cs.a2, cs.off, cs.inc, nrows, cs.nbls, cs.nant, cal.grad);
            hipLaunchKernelGGL((k_jones_weight_rows<T, NP>), dim3(cs.nblk_jones, rows_y), dim3(256), cs.shm, on, wp, vis, weights,
                               cal.x, cal.dx, cs.a1, cs.a2, nrows, cs.nbls, cs.nant, cs.lds_x, cs.lds_dx, vec, cal.terms, rs.bad);
        } else if (!none) {
            if (cal.grad)
                hipLaunchKernelGGL((k_gain_weight_gather<T, NP>), gather, dim3(256), 0, on, wp, (const cplx<T> *)vis, weights, cal.x,
                                   cal.dx, cs.a1, cs.a2, cs.off, cs.inc, nrows, cs.nbls, cs.tpol, cs.nant, cal.grad);
            hipLaunchKernelGGL((k_weight_rows<T, NP, true>), grid, dim3(256), cs.shm, on, wp, vis, weights, cal.x, cal.dx, cs.a1, cs.a2,
                               nrows, L, cs.nbls, cs.nant, cs.nfeed, cs.lds_x, vec, rs.partials, rs.bad);
        } else if constexpr (NP > 0) {  // (without a calibration there is no instance for no parts)
            hipLaunchKernelGGL((k_weight_rows<T, NP, false>), grid, dim3(256), cs.shm, on, wp, vis, weights, cal.x, cal.dx, cs.a1,
                               cs.a2, nrows, L, cs.nbls, cs.nant, cs.nfeed, cs.lds_x, vec, rs.partials, rs.bad);
        }
    });
    if (jones) hipLaunchKernelGGL(k_jones_rows_sum<T>, grid, dim3(256), 0, on, (const double *)cal.terms, nrows, L, rs.partials, rs.bad);
    hipLaunchKernelGGL(k_chi2_rows_reduce, dim3((unsigned)cdiv(nrows, 256)), dim3(256), 0, on, (const double *)rs.partials, nrows,
                       rs.nblk, rs.sums);
}

}  // namespace fv
