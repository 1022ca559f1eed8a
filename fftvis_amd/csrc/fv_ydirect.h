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
// blocks), one transform of one frequency of the group, and a slice of the rows.  Per tile of YD_RT rows it
//   (a) moves the range's distinct column blocks of B (whole blocks: rows of a block are contiguous) from the registers
//       they were loaded into to LDS, and at once requests the next tile's -- that request is outstanding during (b), (c),
//   (b) contracts each group's w columns into D[group][row],
//   (c) lets every thread carry exp(i theta row) for its <= YD_PTM walk slots by multiplication -- re-seeded from sincos
//       every YD_RESEED rows -- and add D's rows from LDS,
// and at the end writes one partial sum per (row slice, transform, point); the gather adds the slices in order.
//
// Walk slots: a point (u, v) and its mirror image (u, -v) in the same u-group read the same column D with conjugate
// phases.  With D = a + i b and exp(i theta (row - na_y / 2)) = c + i s, the four real sums
//     P = sum a c,   Q = sum b s,   R = sum a s,   S = sum b c
// give both values: (P - Q) + i (R + S) at +theta and (P + Q) + i (S - R) at -theta.  Per row that is the four FMAs and
// the phase step one point costs, so a slot -- a pair, or a single point whose second value is not written -- is the
// unit of the walk.  A range's slots are numbered from 0, so occupied slots fill the waves from the front and the waves
// past them skip the walk.  (theta_v = h_y s_v - beta with beta = h_y s_c,v the same for every point: off centre, D
// takes the factor exp(-i beta (row - na_y / 2)) as it is contracted, and theta is h_y s_v alone.  Packed runs are
// centred: beta = 0 and D is the plain contraction.)
// All tables are host-built per (targets, group geometry): Sim::ydirect_plan.
#pragma once

#include "fv_eskernel.h"

namespace fv {

constexpr int YD_THREADS = 512;
constexpr int YD_RT = 32;       // rows per tile
constexpr int YD_NG = 8;        // u-groups per workgroup: YD_NG * YD_RT contraction items, re and im on a thread each
constexpr int YD_PTM = 2;       // walk slots per thread
constexpr int YD_NBMAX = 20;    // distinct column blocks per workgroup (table width)
constexpr int YD_RAWROW = 100;  // LDS cells per tile row: blocks * (block elements + 1 of padding) <= this
constexpr int YD_RAW = YD_RAWROW * YD_RT;
constexpr int YD_NLD = 5;       // cells of a tile a thread loads: blocks * block elements <= YD_NLD * YD_THREADS / YD_RT
constexpr int YD_RESEED = 128;  // rows between two sincos seeds of a point's phase (a multiple of YD_RT)
constexpr int YD_WCH = 4;       // footprint cells the contraction requests from LDS at a time
constexpr int YD_RCH = 4;       // rows of D the walk requests from LDS at a time
static_assert(2 * YD_NG * YD_RT == YD_THREADS, "one contraction item per pair of threads");
static_assert(YD_RESEED % YD_RT == 0, "seeds fall on tile starts");
static_assert(YD_RT == 32 && YD_RT % YD_RCH == 0, "a tile row index is five bits (k_ydirect's shifts)");
static_assert(MAX_W % YD_WCH == 0, "whole chunks of footprint cells");
static_assert(YD_PTM <= 4 && YD_NG * YD_RT / YD_RCH <= 256, "a byte per slot holds its place in D (k_ydirect's dofs)");

// distinct column blocks of 1 << blk elements a workgroup's tile holds (the range builder of Sim::ydirect_plan and the kernel)
__host__ __device__ constexpr int yd_nbcap(int blk) {
    const int a = YD_RAWROW / ((1 << blk) + 1), b = (YD_NLD * YD_THREADS / YD_RT) >> blk;
    return a < b ? (a < YD_NBMAX ? a : YD_NBMAX) : (b < YD_NBMAX ? b : YD_NBMAX);
}

struct YdArgs {
    int w, nfg, nwg, ngroups;
    int na_y, xp;         // rows of B; elements of a row of B (b_pitch)
    int blk;              // log2 of the block width in elements (plain planes: pseudo-blocks of 4 inside a row)
    int64_t blk_stride, row_stride;  // element (bid, row, el) of a plane sits at bid blk_stride + row row_stride + el
    int rps, nslices;     // rows per slice (whole tiles), slices
    int tg;               // transforms per frequency
    int64_t plane;        // elements between two transforms of B (below 2^31: the kernel's cell offsets are 32-bit)
    int64_t npts;         // evaluation points
    double hy, btcy;
    const int *wg;        // [nwg][4]: first group, groups, first slot, slots
    const int *blkcnt;    // [nfg][nwg] distinct blocks
    const int *blkid;     // [nfg][nwg][YD_NBMAX]
    const int *cref;      // [nfg][ngroups][w]: (block slot << 4) | element inside the block
    const double *xw;     // [nfg][ngroups][w] x-kernel weights of the group's footprint
    const double *slv;    // [slots] base v of the slot's phase: its +v point's (a single: its own)
    const int *slg;       // [slots] its u-group
    const int *slp;       // [slots][2] the point at +theta, the point at -theta or -1
};

inline size_t yd_smem_bytes() {
    return sizeof(cplx<double>) * (size_t)(YD_RAW + YD_NG * YD_RT + YD_THREADS + 1) + sizeof(double) * (YD_NG * MAX_W + YD_PTM * YD_THREADS) +
           sizeof(int) * (YD_NG * MAX_W + YD_NBMAX);
}

__global__ __launch_bounds__(YD_THREADS, 4) void k_ydirect(const cplx<double> *__restrict__ B, const double *__restrict__ scale,
                                                          YdArgs a, cplx<double> *__restrict__ vals) {
    extern __shared__ __attribute__((aligned(16))) unsigned char yd_smem[];
    cplx<double> *raw = reinterpret_cast<cplx<double> *>(yd_smem);
    cplx<double> *D = raw + YD_RAW;
    cplx<double> *rot_s = D + YD_NG * YD_RT;  // off-centre launches: the contraction's phase factors (below)
    double *xw_s = reinterpret_cast<double *>(rot_s + YD_THREADS + 1);
    double *th_s = xw_s + YD_NG * MAX_W;  // the slots' phase steps: read back at every seed, so not held in registers
    int *cref_s = reinterpret_cast<int *>(th_s + YD_PTM * YD_THREADS);
    int *bid_s = cref_s + YD_NG * MAX_W;
    const int tid = threadIdx.x, wgi = blockIdx.x, ft = blockIdx.y, fg = ft / a.tg, sl = blockIdx.z;  // ft: (frequency, transform)
    const int g0 = a.wg[4 * wgi], ng = min(a.wg[4 * wgi + 1], YD_NG), p0 = a.wg[4 * wgi + 2],
              np = min(a.wg[4 * wgi + 3], YD_THREADS * YD_PTM);
    const int BE = 1 << a.blk, BEP = BE + 1;
    const int nb = min(a.blkcnt[fg * a.nwg + wgi], yd_nbcap(a.blk));
    const int rbeg = sl * a.rps, rend = min(a.na_y, rbeg + a.rps);
    for (int i = tid; i < ng * a.w; i += YD_THREADS) {
        const int gi = i / a.w, g = i - gi * a.w;
        const int64_t src = ((int64_t)fg * a.ngroups + g0 + gi) * a.w + g;
        const int c = a.cref[src];
        xw_s[gi * MAX_W + g] = a.xw[src];
        // where the cell's tile row 0 sits in raw, in bytes: the contraction adds its row and its half
        cref_s[gi * MAX_W + g] = (min(c >> 4, nb - 1) * YD_RT * BEP + (c & (BE - 1))) * (int)sizeof(cplx<double>);
    }
    if (tid < nb) bid_s[tid] = a.blkid[((int64_t)fg * a.nwg + wgi) * YD_NBMAX + tid];
    // this thread's walk slots: phase step, place of its group's D rows
    const double sc = scale[fg];
    const double beta = a.hy * (sc * a.btcy);  // the centre's share of every phase: taken out of D (below), not carried by the slots
    if (beta != 0.0) {
        // rot_s[tid] = exp(i beta (row - na_y / 2)) for this thread's contraction row of the slice's first tile, stepped
        // a tile at a time by rot_s[YD_THREADS] (a slice has at most some hundred tiles: no seeds in between)
        cplx<double> f;
        sincos(beta * (double)(sl * a.rps + (tid >> 1) % YD_RT - a.na_y / 2), &f.im, &f.re);
        rot_s[tid] = f;
        if (tid == 0) {
            sincos(beta * (double)YD_RT, &f.im, &f.re);
            rot_s[YD_THREADS] = f;
        }
    }
    double dr[YD_PTM], di[YD_PTM], er[YD_PTM], ei[YD_PTM], sp[YD_PTM], sq[YD_PTM], sr[YD_PTM], ss[YD_PTM];
    unsigned dofs = 0;  // a byte per slot: the first of its group's D rows, in units of YD_RCH
    bool kon[YD_PTM];  // wave-uniform: some lane of this wave owns a k-th slot
#pragma unroll
    for (int k = 0; k < YD_PTM; ++k) {
        const int p = tid + k * YD_THREADS;
        kon[k] = k * YD_THREADS + (tid & ~63) < np;
        const int gp = p0 + (p < np ? p : 0);
        const double th = a.hy * (sc * a.slv[gp]);
        th_s[p] = th;  // (read by this thread alone)
        dofs |= (unsigned)(min(max(a.slg[gp] - g0, 0), YD_NG - 1) * (YD_RT / YD_RCH)) << (8 * k);
        sincos(th, &di[k], &dr[k]);
        er[k] = 1.0;
        ei[k] = 0.0;
        sp[k] = sq[k] = sr[k] = ss[k] = 0.0;
    }
    const int citem = tid >> 1, cpart = tid & 1;  // this thread's contraction item, and its half of it: re or im
    // (a wave's 64 threads are the 32 rows of ONE group: its number is wave-uniform and kept in a scalar register)
    const int cgi = __builtin_amdgcn_readfirstlane(citem / YD_RT), crow = citem % YD_RT;
    const int half = a.na_y / 2;
    const int per = YD_RT << a.blk, pshift = a.blk + 5;  // cells of a block's tile rows (YD_RT = 32)
    __syncthreads();  // the tables are in place
    // This thread's YD_NLD cells of a tile.  A block's tile rows are `per` cells and per divides YD_THREADS (2 <= blk <= 4),
    // so the cells share their tile row and block element and sit YD_THREADS / per blocks apart: one row, one place in
    // LDS and a fixed step, and per cell the offset in the plane of B relative to the tile's first row -- the same for
    // every tile.  A cell past the range's blocks or the row's end has no bit in `live`: it loads the tile's first cell
    // instead and zero is stored for it.  Every slot lies inside raw.
    const int lrow = (tid & (per - 1)) >> a.blk, lel = tid & (BE - 1), lbstep = YD_THREADS >> pshift;
    const int lofs = ((tid >> pshift) * YD_RT + lrow) * BEP + lel, lstep = lbstep * YD_RT * BEP;
    unsigned goff[YD_NLD], live = 0;
#pragma unroll
    for (int j = 0; j < YD_NLD; ++j) {
        const int lb = (tid >> pshift) + j * lbstep;
        goff[j] = 0;
        if (lb < nb) {
            const int bid = bid_s[lb];
            if ((bid << a.blk) + lel < a.xp) {
                goff[j] = (unsigned)((int64_t)bid * a.blk_stride + (int64_t)lrow * a.row_stride + lel);
                live |= 1u << j;
            }
        }
    }
    // Tile r0 stores its cells -- requested one tile earlier -- to LDS and requests the next tile's before it contracts
    // and walks, so a whole request is outstanding under both.  (The loop starts one tile early so that the load
    // sequence exists once; the first trip only requests.)
    const cplx<double> *plane = B + (int64_t)ft * a.plane;
    cplx<double> pf[YD_NLD];
    for (int r0 = rbeg - YD_RT; r0 < rend; r0 += YD_RT) {
        if (r0 >= rbeg) {
            // (the last contraction's reads of raw ended before its barrier; the barrier below ends the last walk's of D)
            const unsigned ok = r0 + lrow < rend ? live : 0;
#pragma unroll
            for (int j = 0; j < YD_NLD; ++j) raw[lofs + j * lstep] = (ok >> j) & 1 ? pf[j] : cplx<double>{0.0, 0.0};
        }
        if (r0 + YD_RT < rend) {
            const cplx<double> *base = plane + (int64_t)(r0 + YD_RT) * a.row_stride;  // uniform; a row below rend
            const bool rowin = r0 + YD_RT + lrow < rend;
#pragma unroll
            for (int j = 0; j < YD_NLD; ++j) pf[j] = base[rowin ? goff[j] : 0u];
        }
        if (r0 < rbeg) continue;
        __syncthreads();
        if (cgi < ng) {  // D[group][row] = sum over the footprint, cells in increasing g; YD_WCH requested at a time
            const char *mine = reinterpret_cast<const char *>(raw) + (crow * BEP * 2 + cpart) * (int)sizeof(double);
            double sum = 0.0;
            for (int gb = 0; gb < a.w; gb += YD_WCH) {
                int c[YD_WCH];
                double wv[YD_WCH], v[YD_WCH];
#pragma unroll
                for (int q = 0; q < YD_WCH; ++q) {
                    c[q] = cref_s[cgi * MAX_W + gb + q];
                    wv[q] = xw_s[cgi * MAX_W + gb + q];
                }
#pragma unroll
                for (int q = 0; q < YD_WCH; ++q)  // (table cells past w are never written: cell 0 then, unused)
                    v[q] = *reinterpret_cast<const double *>(mine + (gb + q < a.w ? c[q] : 0));
#pragma unroll
                for (int q = 0; q < YD_WCH; ++q)
                    if (gb + q < a.w) sum += v[q] * wv[q];
            }
            if (beta != 0.0) {  // uniform; D[row] exp(-i beta (row - na_y / 2)): the partner thread holds the other half
                const cplx<double> f = rot_s[tid], st = rot_s[YD_THREADS];
                const double other = __shfl_xor(sum, 1);
                sum = cpart ? sum * f.re - other * f.im : sum * f.re + other * f.im;
                rot_s[tid] = {f.re * st.re - f.im * st.im, f.re * st.im + f.im * st.re};  // the next tile's
            }
            reinterpret_cast<double *>(D)[2 * (cgi * YD_RT + crow) + cpart] = sum;
        }
        __syncthreads();
        if ((r0 - rbeg) % YD_RESEED == 0) {
#pragma unroll
            for (int k = 0; k < YD_PTM; ++k)
                if (kon[k]) sincos(th_s[tid + k * YD_THREADS] * (double)(r0 - half), &ei[k], &er[k]);
        }
#pragma unroll
        for (int k = 0; k < YD_PTM; ++k) {
            if (!kon[k]) continue;  // wave-uniform
            const cplx<double> *d = D + ((dofs >> (8 * k)) & 255u) * YD_RCH;
#pragma unroll 1
            for (int rb = 0; rb < YD_RT; rb += YD_RCH) {  // YD_RCH rows of D requested at a time
                cplx<double> v[YD_RCH];
#pragma unroll
                for (int q = 0; q < YD_RCH; ++q) v[q] = d[rb + q];
#pragma unroll
                for (int q = 0; q < YD_RCH; ++q) {
                    sp[k] += v[q].re * er[k];
                    sq[k] += v[q].im * ei[k];
                    sr[k] += v[q].re * ei[k];
                    ss[k] += v[q].im * er[k];
                    const double e2 = er[k] * dr[k] - ei[k] * di[k];
                    ei[k] = er[k] * di[k] + ei[k] * dr[k];
                    er[k] = e2;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < YD_PTM; ++k) {
        const int p = tid + k * YD_THREADS;
        if (p >= np) continue;
        cplx<double> *out = vals + ((int64_t)sl * a.nfg * a.tg + ft) * a.npts;
        const int pp = a.slp[2 * (p0 + p)], pm = a.slp[2 * (p0 + p) + 1];
        if (pp >= 0 && pp < a.npts) out[pp] = {sp[k] - sq[k], sr[k] + ss[k]};
        if (pm >= 0 && pm < a.npts) out[pm] = {sp[k] + sq[k], ss[k] - sr[k]};
    }
}

// a table of ones in place of the inner deconvolution along y (the spread kernels take a table per dimension)
__global__ void k_yd_ones(double *__restrict__ tab, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab[i] = 1.0;
}

}  // namespace fv
