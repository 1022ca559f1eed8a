// fv_ydirect.h -- exact y sums over contracted u-columns (type-3 forward on lattice arrays).
//
// The evaluation points of a regular array sit on few distinct u values (HERA-350: 11 916 points, both signs, on 173).
// For such targets the second dimension needs neither its FFT pass, nor the grid C, nor an interpolation: the w columns
// of the x-pass output B that one u-footprint reads are contracted with the x-kernel weights into ONE column
//     D_u[row] = sum_g kx[g] B[row][col(j0 + g)],        row in [0, na_y),
// and the transform at a target (u, v) is the exact sum
//     sum_row D_u[row] exp(i theta_v (row - na_y / 2)),   theta_v = h_y (s_v - s_c,v),
// the same convention as the pruned FFT (k_rowfft_*: inverse sign, input centred on na / 2).  The spread applies no
// inner deconvolution along y on such launches (there is no inner kernel to undo); the gather's values variant
// (k_interp<.., VALS>) still divides by the source kernel's transform in BOTH dimensions, like Nufft3::zdirect does for z.
//
// Work split: a workgroup takes a range of adjacent u-groups (<= YD_NG; their footprints share B's 64-byte column
// blocks), one frequency of the group with all its transforms, and a slice of the rows.  Per tile of YD_RT rows it
//   (a) streams the range's distinct column blocks of B through LDS (whole blocks: rows of a block are contiguous) and
//       contracts each group's w columns into D[group][row][transform],
//   (b) lets every thread carry exp(i theta row) for its <= YD_PTM points by multiplication -- re-seeded from sincos
//       every YD_RESEED rows -- and add D's rows from LDS,
//   (c) and at the end writes one partial sum per (row slice, transform, point); the gather adds the slices in order.
// All tables are host-built per (targets, group geometry): Sim::ydirect_plan.
#pragma once

#include "fv_eskernel.h"

namespace fv {

constexpr int YD_THREADS = 256;
constexpr int YD_RT = 32;       // rows per tile
constexpr int YD_NG = 8;        // u-groups per workgroup: YD_NG * YD_RT contraction items = one per thread
constexpr int YD_PTM = 4;       // evaluation points per thread
constexpr int YD_NBMAX = 20;    // distinct column blocks per workgroup (table width)
constexpr int YD_RAWROW = 100;  // LDS cells per tile row: blocks * (block elements + 1 of padding) <= this
constexpr int YD_RAW = YD_RAWROW * YD_RT;
constexpr int YD_NLD = 11;      // cells of a tile a thread loads per transform: blocks * block elements <= 8 YD_NLD
constexpr int YD_RESEED = 128;  // rows between two sincos seeds of a point's phase (a multiple of YD_RT)
static_assert(YD_NG * YD_RT == YD_THREADS, "one contraction item per thread");
static_assert(YD_RESEED % YD_RT == 0, "seeds fall on tile starts");
static_assert(YD_RT == 32, "a tile row index is five bits (k_ydirect's shifts)");

struct YdArgs {
    int w, nfg, nwg, ngroups;
    int na_y, xp;         // rows of B; elements of a row of B (b_pitch)
    int blk;              // log2 of the block width in elements (plain planes: pseudo-blocks of 4 inside a row)
    int64_t blk_stride, row_stride;  // element (bid, row, el) of a plane sits at bid blk_stride + row row_stride + el
    int rps, nslices;     // rows per slice (whole tiles), slices
    int64_t plane;        // elements between two transforms of B
    int64_t npts;         // evaluation points
    double hy, btcy;
    const int *wg;        // [nwg][4]: first group, groups, first point, points
    const int *blkcnt;    // [nfg][nwg] distinct blocks
    const int *blkid;     // [nfg][nwg][YD_NBMAX]
    const int *cref;      // [nfg][ngroups][w]: (block slot << 4) | element inside the block
    const double *xw;     // [nfg][ngroups][w] x-kernel weights of the group's footprint
    const double *ptv;    // [npts] sign-adjusted base v of every point
    const int *ptg;       // [npts] its u-group
};

inline size_t yd_smem_bytes(int tg) {
    return sizeof(cplx<double>) * (size_t)(YD_RAW + YD_NG * YD_RT * tg) + sizeof(double) * YD_NG * MAX_W +
           sizeof(int) * (YD_NG * MAX_W + YD_NBMAX);
}

template <int TG>
__global__ __launch_bounds__(YD_THREADS, 2) void k_ydirect(const cplx<double> *__restrict__ B, const double *__restrict__ scale,
                                                          YdArgs a, cplx<double> *__restrict__ vals) {
    extern __shared__ __attribute__((aligned(16))) unsigned char yd_smem[];
    cplx<double> *raw = reinterpret_cast<cplx<double> *>(yd_smem);
    cplx<double> *D = raw + YD_RAW;
    double *xw_s = reinterpret_cast<double *>(D + YD_NG * YD_RT * TG);
    int *cref_s = reinterpret_cast<int *>(xw_s + YD_NG * MAX_W);
    int *bid_s = cref_s + YD_NG * MAX_W;
    const int tid = threadIdx.x, wgi = blockIdx.x, fg = blockIdx.y, sl = blockIdx.z;
    const int g0 = a.wg[4 * wgi], ng = min(a.wg[4 * wgi + 1], YD_NG), p0 = a.wg[4 * wgi + 2],
              np = min(a.wg[4 * wgi + 3], YD_THREADS * YD_PTM);
    const int BE = 1 << a.blk, BEP = BE + 1;
    const int nb = min(a.blkcnt[fg * a.nwg + wgi], min(YD_NBMAX, min(YD_RAWROW / BEP, (8 * YD_NLD) >> a.blk)));
    const int rbeg = sl * a.rps, rend = min(a.na_y, rbeg + a.rps);
    for (int i = tid; i < ng * a.w; i += YD_THREADS) {
        const int gi = i / a.w, g = i - gi * a.w;
        const int64_t src = ((int64_t)fg * a.ngroups + g0 + gi) * a.w + g;
        xw_s[gi * MAX_W + g] = a.xw[src];
        cref_s[gi * MAX_W + g] = a.cref[src];
    }
    if (tid < nb) bid_s[tid] = a.blkid[((int64_t)fg * a.nwg + wgi) * YD_NBMAX + tid];
    // this thread's points: phase step, slot of its group's D rows
    const double sc = scale[fg];
    double th[YD_PTM], dr[YD_PTM], di[YD_PTM], er[YD_PTM], ei[YD_PTM], accr[YD_PTM][TG], acci[YD_PTM][TG];
    int dofs[YD_PTM];
    bool kon[YD_PTM];  // wave-uniform: some lane of this wave owns a k-th point
#pragma unroll
    for (int k = 0; k < YD_PTM; ++k) {
        const int p = tid + k * YD_THREADS;
        kon[k] = k * YD_THREADS + (tid & ~63) < np;
        const int gp = p0 + (p < np ? p : 0);
        th[k] = a.hy * (sc * a.ptv[gp] - sc * a.btcy);
        dofs[k] = min(max(a.ptg[gp] - g0, 0), YD_NG - 1) * YD_RT * TG;
        sincos(th[k], &di[k], &dr[k]);
        er[k] = 1.0;
        ei[k] = 0.0;
#pragma unroll
        for (int t = 0; t < TG; ++t) accr[k][t] = acci[k][t] = 0.0;
    }
    const int cgi = tid / YD_RT, crow = tid % YD_RT;  // this thread's contraction item
    const int half = a.na_y / 2;
    const int per = YD_RT << a.blk, pshift = a.blk + 5;  // cells of a block's tile rows (YD_RT = 32)
    const int nitems = min(nb * per, YD_NLD * YD_THREADS);
    // A tile's cells of one transform, YD_NLD per thread: every load is issued before the first one is used, and the
    // next (tile, transform)'s are issued as soon as this one's have gone to LDS -- in flight under the contraction
    // and the sums.  (One load per loop trip, each waited for, cost ten memory round trips per tile and transform.)
    cplx<double> pf[YD_NLD];
    auto issue = [&](int r0, int t) {
        const cplx<double> *pl = B + ((int64_t)fg * TG + t) * a.plane;
#pragma unroll
        for (int j = 0; j < YD_NLD; ++j) {
            const int i = tid + j * YD_THREADS;
            const int lb = i >> pshift, rem = i & (per - 1), row = rem >> a.blk, el = rem & (BE - 1);
            pf[j] = {0.0, 0.0};
            if (i < nitems) {
                const int bid = bid_s[lb];
                if (r0 + row < rend && (bid << a.blk) + el < a.xp)
                    pf[j] = pl[(int64_t)bid * a.blk_stride + (int64_t)(r0 + row) * a.row_stride + el];
            }
        }
    };
    __syncthreads();  // the tables are in place
    if (rbeg < rend) issue(rbeg, 0);
    for (int r0 = rbeg, tile = 0; r0 < rend; r0 += YD_RT, ++tile) {
        for (int t = 0; t < TG; ++t) {
            __syncthreads();  // the last contraction has read its raw cells, the last tile's sums their D rows
#pragma unroll
            for (int j = 0; j < YD_NLD; ++j) {
                const int i = tid + j * YD_THREADS;
                const int lb = i >> pshift, rem = i & (per - 1), row = rem >> a.blk, el = rem & (BE - 1);
                if (i < nitems) raw[(lb * YD_RT + row) * BEP + el] = pf[j];
            }
            {
                const int nt = t + 1 < TG ? t + 1 : 0, nr0 = t + 1 < TG ? r0 : r0 + YD_RT;
                if (nr0 < rend) issue(nr0, nt);
            }
            __syncthreads();
            if (cgi < ng) {
                double sr = 0.0, si = 0.0;
                for (int g = 0; g < a.w; ++g) {
                    const int c = cref_s[cgi * MAX_W + g];
                    const cplx<double> v = raw[(min(c >> 4, nb - 1) * YD_RT + crow) * BEP + (c & (BE - 1))];
                    const double wv = xw_s[cgi * MAX_W + g];
                    sr += v.re * wv;
                    si += v.im * wv;
                }
                D[(cgi * YD_RT + crow) * TG + t] = {sr, si};
            }
        }
        __syncthreads();
        if (tile % (YD_RESEED / YD_RT) == 0) {
#pragma unroll
            for (int k = 0; k < YD_PTM; ++k)
                if (kon[k]) sincos(th[k] * (double)(r0 - half), &ei[k], &er[k]);
        }
#pragma unroll 2
        for (int row = 0; row < YD_RT; ++row) {
#pragma unroll
            for (int k = 0; k < YD_PTM; ++k) {
                if (!kon[k]) continue;  // wave-uniform
                const cplx<double> *d = D + dofs[k] + row * TG;
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    const cplx<double> v = d[t];
                    accr[k][t] += v.re * er[k] - v.im * ei[k];
                    acci[k][t] += v.re * ei[k] + v.im * er[k];
                }
                const double e2 = er[k] * dr[k] - ei[k] * di[k];
                ei[k] = er[k] * di[k] + ei[k] * dr[k];
                er[k] = e2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < YD_PTM; ++k) {
        const int p = tid + k * YD_THREADS;
        if (p >= np) continue;
#pragma unroll
        for (int t = 0; t < TG; ++t)
            vals[(((int64_t)sl * a.nfg + fg) * TG + t) * a.npts + p0 + p] = {accr[k][t], acci[k][t]};
    }
}

// a table of ones in place of the inner deconvolution along y (the spread kernels take a table per dimension)
__global__ void k_yd_ones(double *__restrict__ tab, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab[i] = 1.0;
}

}  // namespace fv
