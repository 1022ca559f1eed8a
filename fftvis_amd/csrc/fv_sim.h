// fv_sim.h -- the fused visibility simulator: per time  rotate -> horizon compaction -> az/za;
// per frequency group  beam x coherency strengths -> type-3 NUFFT (spread, pruned row FFTs, gather).
//
// GPU twin of CPUSimulationEngine._evaluate_vis_chunk (src/fftvis/cpu/cpu_simulate.py:856-1071).
// Loop order follows the reference (time -> frequency -> beam pair); what differs is that a
// block of neighbouring frequencies shares one fine grid geometry, so their strengths ride one
// spread launch and one batched FFT as extra "transforms" (DESIGN.md "Frequency groups").
// The fit layer's kernels and launchers (objective, Gauss-Newton weighting, gains, Jones matrices, the solves) are in
// fv_fit.h; the engine's two row-pass bodies, Sim::residual_pass and Sim::weight_pass, launch them on a handle's block.
#pragma once

#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>
#include "fv_fit.h"
#include "fv_nufft.h"
#include <unordered_map>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <memory>

namespace fv {

constexpr double SPEED_OF_LIGHT = 299792458.0;  // core/utils.py:9

struct BeamDesc {
    int kind;            // 0 Airy, 1 table
    int order;           // tables: interpolation order 0..5 (read by the general-order path only, eval_* <ORD = 0>)
    double diameter;     // Airy
    double js[8];        // Airy: complex factor per Jones slot A[ax][feed] = js . 2 J1(x)/x  (re, im pairs)
    double ps;           // Airy: factor of the power beam, ps . (2 J1(x)/x)^2
    const void *table;   // device
    int nfreq_tab, nza, naz;
    double za_max;
};

// ---------------------------------------------------------------------------------------------
// per-time kernels
// ---------------------------------------------------------------------------------------------
struct Rot9 {
    double m[9];
};

// Pass 1: above-horizon flag count per 256-source block (select_chunk's up > 0,
// cpu_simulate.py:940-946 via matvis).
// The kernels work on the source range [off, off + n) of the catalog (eq is (3, stride) SoA): one
// source chunk of the reference's `for chunk in range(nchunks)` loop (cpu_simulate.py:939).
template <typename T>
__global__ void k_horizon_count(int64_t n, int64_t stride, int64_t off, const T *__restrict__ eq, Rot9 rt,
                                int *__restrict__ block_counts) {
    __shared__ int wsum[4];
    int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool up = false;
    if (j < n) {
        double ex = eq[off + j], ey = eq[stride + off + j], ez = eq[2 * stride + off + j];
        up = rt.m[6] * ex + rt.m[7] * ey + rt.m[8] * ez > 0.0;
    }
    unsigned long long b = __ballot(up);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Pass 2: stable compaction + everything that depends only on (time, source):
//   topo = R_t eq;  az, za in the UN-rotated ENU frame (cpu_simulate.py:957-959, matvis
//   enu_to_az_za "uvbeam");  x = 2 pi R_plane topo (cpu_simulate.py:961-967).
// cap = capacity of the compacted arrays (chunk size x source_buffer): sources beyond it are not
// stored and counted in *overflow (matvis raises likewise when its above-horizon buffer is too small).
template <typename T>
__global__ void k_horizon_compact(int64_t nsrc, int64_t stride, int64_t off, const T *__restrict__ eq, Rot9 rt,
                                  Rot9 rp, const int *__restrict__ block_off, T *__restrict__ xyz,
                                  int64_t cap, T *__restrict__ az, T *__restrict__ za,
                                  int *__restrict__ src_idx, int *__restrict__ overflow) {
    __shared__ int wsum[4];
    int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double e = 0, n = 0, u = -1;
    if (j < nsrc) {
        double ex = eq[off + j], ey = eq[stride + off + j], ez = eq[2 * stride + off + j];
        e = rt.m[0] * ex + rt.m[1] * ey + rt.m[2] * ez;
        n = rt.m[3] * ex + rt.m[4] * ey + rt.m[5] * ez;
        u = rt.m[6] * ex + rt.m[7] * ey + rt.m[8] * ez;
    }
    const bool up = j < nsrc && u > 0.0;
    unsigned long long b = __ballot(up);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    int base = block_off[blockIdx.x];
    for (int i = 0; i < wv; ++i) base += wsum[i];
    if (!up) return;
    const int64_t pos = base + __popcll(b & ((1ull << lane) - 1ull));
    if (pos >= cap) {
        atomicAdd(overflow, 1);
        return;
    }
    const double lsqr = n * n + e * e;
    const double zeta = sqrt(fmax(0.0, 1.0 - lsqr));
    double azv = 0.5 * M_PI - atan2(e, n);
    azv = fmod(azv, 2.0 * M_PI);
    if (azv < 0) azv += 2.0 * M_PI;
    az[pos] = (T)azv;
    za[pos] = (T)(0.5 * M_PI - asin(zeta));
    const double twopi = 2.0 * M_PI;
    xyz[pos] = (T)(twopi * (rp.m[0] * e + rp.m[1] * n + rp.m[2] * u));
    xyz[cap + pos] = (T)(twopi * (rp.m[3] * e + rp.m[4] * n + rp.m[5] * u));
    xyz[2 * cap + pos] = (T)(twopi * (rp.m[6] * e + rp.m[7] * n + rp.m[8] * u));
    src_idx[pos] = (int)(off + j);
}

// ---------------------------------------------------------------------------------------------
// beam x coherency  (evaluate_beam cpu/beams.py:12-89; _compute_apparent_coherency
// cpu_simulate.py:90-202; numba kernels cpu/beams.py:129-246)
// ---------------------------------------------------------------------------------------------
__device__ inline double airy_efield(double diameter, double freq, double za) {
    const double x = M_PI * diameter * freq * sin(za) / SPEED_OF_LIGHT;
    return x == 0.0 ? 1.0 : 2.0 * j1(x) / x;
}

struct Bilin {
    int ia0, ia1, iz0, iz1;
    double wa, wz;
};

__device__ inline Bilin bilin_setup(const BeamDesc &b, double az, double za) {
    Bilin o;
    const double twopi = 2.0 * M_PI;
    double a = fmod(az, twopi);
    if (a < 0) a += twopi;
    const double fa = a / (twopi / b.naz);
    int ia0 = (int)floor(fa);
    o.wa = fa - ia0;
    ia0 %= b.naz;
    o.ia0 = ia0;
    o.ia1 = (ia0 + 1) % b.naz;
    double fz = za / (b.za_max / (b.nza - 1));
    fz = fmin(fmax(fz, 0.0), (double)(b.nza - 1));
    int iz0 = min((int)floor(fz), b.nza - 2);
    o.wz = fz - iz0;
    o.iz0 = iz0;
    o.iz1 = iz0 + 1;
    return o;
}

// Order-3 interpolation (beam_spline_opts {"order": 3}, the reference CLI's default, cli.py:50,146;
// scipy.ndimage.map_coordinates semantics: interpolating cubic B-spline): nodes floor(x) - 1 .. + 2
// with the B-spline weights, on a table whose samples were replaced by spline coefficients at upload
// (k_bspline3_prefilter).  az is periodic; za mirrors about its first and last node.
struct Cubic {
    int ia[4], iz[4];
    double wa[4], wz[4];
};

__device__ inline void bspline3_weights(double t, double w[4]) {
    const double u = 1.0 - t, t2 = t * t, t3 = t2 * t;
    w[0] = u * u * u * (1.0 / 6.0);
    w[1] = (4.0 - 6.0 * t2 + 3.0 * t3) * (1.0 / 6.0);
    w[2] = (1.0 + 3.0 * t + 3.0 * t2 - 3.0 * t3) * (1.0 / 6.0);
    w[3] = t3 * (1.0 / 6.0);
}

__device__ inline Cubic cubic_setup(const BeamDesc &b, double az, double za) {
    Cubic o;
    const double twopi = 2.0 * M_PI;
    double a = fmod(az, twopi);
    if (a < 0) a += twopi;
    const double fa = a / (twopi / b.naz);
    const int ia0 = (int)floor(fa);
    bspline3_weights(fa - ia0, o.wa);
    for (int k = 0; k < 4; ++k) o.ia[k] = ((ia0 - 1 + k) % b.naz + b.naz) % b.naz;
    double fz = za / (b.za_max / (b.nza - 1));
    fz = fmin(fmax(fz, 0.0), (double)(b.nza - 1));
    const int iz0 = min((int)floor(fz), b.nza - 2);
    bspline3_weights(fz - iz0, o.wz);
    const int per = 2 * (b.nza - 1);
    for (int k = 0; k < 4; ++k) {
        int j = ((iz0 - 1 + k) % per + per) % per;
        o.iz[k] = j < b.nza ? j : per - j;
    }
    return o;
}

// Any order 0 .. 5 (beam_spline_opts {"order": n}; scipy.ndimage.map_coordinates semantics as for order 3): the
// n + 1 nodes start at floor(x) - n / 2 (odd n) or floor(x + 1/2) - n / 2 (even n: the centred B-spline's knots sit
// at half-integers) and carry the cardinal B-spline's values, built by the Cox - de Boor triangle on uniform knots
// (every denominator is the level j).  Orders 1 and 3 have their own unrolled paths above; this one runs the
// others (0: nearest node; 2, 4, 5: on coefficients from k_bspline_prefilter) with the order read at run time.
struct SplineN {
    int n;  // order
    int ia[6], iz[6];
    double wa[6], wz[6];
};

__device__ inline void bspline_weights(int n, double t, double w[6]) {  // t in [0, 1]: position inside the knot span
    w[0] = 1.0;
    for (int j = 1; j <= n; ++j) {
        double saved = 0.0;
        const double inv = 1.0 / j;
        for (int r = 0; r < j; ++r) {
            const double right = r + 1 - t, left = t + (j - r - 1);
            const double tmp = w[r] * inv;
            w[r] = saved + right * tmp;
            saved = left * tmp;
        }
        w[j] = saved;
    }
}

__device__ inline SplineN spline_setup(const BeamDesc &b, double az, double za) {
    SplineN o;
    const int n = o.n = b.order;
    const double half = n & 1 ? 0.0 : 0.5;
    const double twopi = 2.0 * M_PI;
    double a = fmod(az, twopi);
    if (a < 0) a += twopi;
    const double fa = a / (twopi / b.naz) + half;
    const int ia0 = (int)floor(fa);
    bspline_weights(n, fa - ia0, o.wa);
    for (int k = 0; k <= n; ++k) o.ia[k] = ((ia0 - n / 2 + k) % b.naz + b.naz) % b.naz;
    double fz = za / (b.za_max / (b.nza - 1));
    fz = fmin(fmax(fz, 0.0), (double)(b.nza - 1)) + half;
    const int iz0 = n & 1 ? min((int)floor(fz), b.nza - 2) : (int)floor(fz);
    bspline_weights(n, fz - iz0, o.wz);
    const int per = 2 * (b.nza - 1);
    for (int k = 0; k <= n; ++k) {
        const int j = ((iz0 - n / 2 + k) % per + per) % per;
        o.iz[k] = j < b.nza ? j : per - j;
    }
    return o;
}

// scipy.ndimage.spline_filter1d(order) in place, one line per thread, on a table stored as
// [freq][za][az][C] doubles: axis 0 = za lines (mode "mirror"), axis 1 = az lines ("grid-wrap").
// One causal + anticausal sweep per pole (order 2: sqrt(8) - 3; 3: sqrt(3) - 2; 4 and 5: two poles each), after the
// gain prod (1 - z)(1 - 1 / z); boundary sums run over the whole line (exact, as scipy's).
__global__ void k_bspline_prefilter(double *__restrict__ data, int64_t nfreq, int nza, int naz, int C,
                                    int axis, int order) {
    const int nother = axis == 0 ? naz : nza;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nfreq * nother * C) return;
    const int c = (int)(t % C);
    const int64_t r = t / C;
    const int other = (int)(r % nother);
    const int64_t f = r / nother;
    double *p;
    int64_t st;
    int n;
    if (axis == 0) {
        p = data + ((f * nza) * naz + other) * C + c;
        st = (int64_t)naz * C;
        n = nza;
    } else {
        p = data + ((f * nza + other) * naz) * C + c;
        st = C;
        n = naz;
    }
    if (n < 2) return;
    double poles[2];
    int npoles = 1;
    switch (order) {
        case 2: poles[0] = sqrt(8.0) - 3.0; break;
        case 3: poles[0] = sqrt(3.0) - 2.0; break;
        case 4:
            npoles = 2;
            poles[0] = sqrt(664.0 - sqrt(438976.0)) + sqrt(304.0) - 19.0;
            poles[1] = sqrt(664.0 + sqrt(438976.0)) - sqrt(304.0) - 19.0;
            break;
        case 5:
            npoles = 2;
            poles[0] = sqrt(67.5 - sqrt(4436.25)) + sqrt(26.25) - 6.5;
            poles[1] = sqrt(67.5 + sqrt(4436.25)) - sqrt(26.25) - 6.5;
            break;
        default: return;  // orders 0 and 1 interpolate the samples themselves
    }
    double gain = 1.0;
    for (int q = 0; q < npoles; ++q) gain *= (1.0 - poles[q]) * (1.0 - 1.0 / poles[q]);
    for (int i = 0; i < n; ++i) p[i * st] *= gain;
    for (int q = 0; q < npoles; ++q) {
    const double z = poles[q];
    if (axis == 0) {  // mirror
        const double zn1 = pow(z, (double)(n - 1));
        double c0 = p[0] + zn1 * p[(n - 1) * st], zi = z;
        for (int i = 1; i < n - 1; ++i) {
            c0 += zi * (p[i * st] + zn1 * p[(n - 1 - i) * st]);
            zi *= z;
        }
        p[0] = c0 / (1.0 - zn1 * zn1);
    } else {  // periodic
        double c0 = p[0], zi = z;
        for (int i = 1; i < n; ++i) {
            c0 += zi * p[(n - i) * st];
            zi *= z;
        }
        p[0] = c0 / (1.0 - zi);
    }
    double prev = p[0];
    for (int i = 1; i < n; ++i) {
        prev = p[i * st] + z * prev;
        p[i * st] = prev;
    }
    if (axis == 0) {
        p[(n - 1) * st] = (z * p[(n - 2) * st] + p[(n - 1) * st]) * z / (z * z - 1.0);
    } else {
        double cl = p[(n - 1) * st], zi = z;
        for (int i = 0; i < n - 1; ++i) {
            cl += zi * p[i * st];
            zi *= z;
        }
        p[(n - 1) * st] = cl * z / (zi - 1.0);
    }
    double next = p[(n - 1) * st];
    for (int i = n - 2; i >= 0; --i) {
        next = z * (next - p[i * st]);
        p[i * st] = next;
    }
    }  // poles
}

// [freq][4][za][az] (caller's layout) -> [freq][za][az][4] (device layout of Jones tables)
__global__ void k_jones_interleave(const cplx<double> *__restrict__ in, cplx<double> *__restrict__ out,
                                   int64_t nodes, int64_t nfreq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nodes * nfreq) return;
    const int64_t f = i / nodes, nd = i % nodes;
    for (int j = 0; j < 4; ++j) out[(f * nodes + nd) * 4 + j] = in[(f * 4 + j) * nodes + nd];
}

// samples -> B-spline coefficients of the given order, both axes (orders >= 2; once per upload)
inline void bspline_prefilter(double *table, int64_t nfreq, int nza, int naz, int C, int order, hipStream_t s) {
    if (order < 2) return;
    for (int axis = 0; axis < 2; ++axis) {
        const int64_t lines = nfreq * (axis == 0 ? naz : nza) * C;
        hipLaunchKernelGGL(k_bspline_prefilter, dim3((unsigned)cdiv(lines, 64)), dim3(64), 0, s, table, nfreq,
                           nza, naz, C, axis, order);
    }
}
// kernel variant for an order: 1 and 3 unrolled, everything else through the general path (template value 0)
inline int beam_order_variant(int order) { return order == 1 || order == 3 ? order : 0; }

// Jones matrix A[ax][feed] (row-major, 4 complex) of one beam at one (source, frequency).
template <int ORD>
__device__ inline void eval_jones(const BeamDesc &b, int fidx, double freq, double az, double za,
                                  cplx<double> A[4]) {
    if (b.kind == 0) {
        const double e = airy_efield(b.diameter, freq, za);
        for (int i = 0; i < 4; ++i) A[i] = {e * b.js[2 * i], e * b.js[2 * i + 1]};
        return;
    }
    const int ft = b.nfreq_tab > 1 ? fidx : 0;
    if (ORD == 0) {
        const SplineN w = spline_setup(b, az, za);
        const cplx<double> *tab = (const cplx<double> *)b.table + (int64_t)ft * 4 * b.nza * b.naz;
        for (int i = 0; i < 4; ++i) A[i] = {0.0, 0.0};
        for (int k = 0; k <= w.n; ++k)
            for (int l = 0; l <= w.n; ++l) {
                const double wt = w.wz[k] * w.wa[l];
                const cplx<double> *nd = tab + ((int64_t)w.iz[k] * b.naz + w.ia[l]) * 4;
                for (int i = 0; i < 4; ++i) {
                    const cplx<double> v = nd[i];
                    A[i].re += v.re * wt;
                    A[i].im += v.im * wt;
                }
            }
        return;
    }
    if (ORD == 3) {
        const Cubic w = cubic_setup(b, az, za);
        const cplx<double> *tab = (const cplx<double> *)b.table + (int64_t)ft * 4 * b.nza * b.naz;
        for (int i = 0; i < 4; ++i) A[i] = {0.0, 0.0};
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 4; ++l) {
                const double wt = w.wz[k] * w.wa[l];
                const cplx<double> *nd = tab + ((int64_t)w.iz[k] * b.naz + w.ia[l]) * 4;
                for (int i = 0; i < 4; ++i) {
                    const cplx<double> v = nd[i];
                    A[i].re += v.re * wt;
                    A[i].im += v.im * wt;
                }
            }
        return;
    }
    const Bilin w = bilin_setup(b, az, za);
    // device layout [freq][za][az][4 Jones]: the four Jones entries of a node are one 64-B sector (the
    // caller's [freq][2][2][za][az] planes are interleaved at upload, k_jones_interleave)
    const cplx<double> *tab = (const cplx<double> *)b.table + (int64_t)ft * 4 * b.nza * b.naz;
    const double w00 = (1 - w.wz) * (1 - w.wa), w01 = (1 - w.wz) * w.wa, w10 = w.wz * (1 - w.wa),
                 w11 = w.wz * w.wa;
    const cplx<double> *n00 = tab + ((int64_t)w.iz0 * b.naz + w.ia0) * 4, *n01 = tab + ((int64_t)w.iz0 * b.naz + w.ia1) * 4,
                       *n10 = tab + ((int64_t)w.iz1 * b.naz + w.ia0) * 4, *n11 = tab + ((int64_t)w.iz1 * b.naz + w.ia1) * 4;
    for (int i = 0; i < 4; ++i) {
        const cplx<double> v00 = n00[i], v01 = n01[i], v10 = n10[i], v11 = n11[i];
        A[i] = {v00.re * w00 + v01.re * w01 + v10.re * w10 + v11.re * w11,
                v00.im * w00 + v01.im * w01 + v10.im * w10 + v11.im * w11};
    }
}

// Power beam (unpolarized path: prepare_beam_unpolarized in wrapper.py:278-279 hands the engine a
// single-polarisation power beam; evaluate_beam returns [0,0,0,:], cpu/beams.py:78-81).
template <int ORD>
__device__ inline double eval_power(const BeamDesc &b, int fidx, double freq, double az, double za) {
    if (b.kind == 0) {
        const double e = airy_efield(b.diameter, freq, za);
        return e * e * b.ps;
    }
    const int ft = b.nfreq_tab > 1 ? fidx : 0;
    const double *p = (const double *)b.table + (int64_t)ft * b.nza * b.naz;
    if (ORD == 0) {
        const SplineN w = spline_setup(b, az, za);
        double acc = 0.0;
        for (int k = 0; k <= w.n; ++k)
            for (int l = 0; l <= w.n; ++l) acc += w.wz[k] * w.wa[l] * p[(int64_t)w.iz[k] * b.naz + w.ia[l]];
        return acc;
    }
    if (ORD == 3) {
        const Cubic w = cubic_setup(b, az, za);
        double acc = 0.0;
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 4; ++l) acc += w.wz[k] * w.wa[l] * p[(int64_t)w.iz[k] * b.naz + w.ia[l]];
        return acc;
    }
    const Bilin w = bilin_setup(b, az, za);
    return p[(int64_t)w.iz0 * b.naz + w.ia0] * (1 - w.wz) * (1 - w.wa) +
           p[(int64_t)w.iz0 * b.naz + w.ia1] * (1 - w.wz) * w.wa +
           p[(int64_t)w.iz1 * b.naz + w.ia0] * w.wz * (1 - w.wa) +
           p[(int64_t)w.iz1 * b.naz + w.ia1] * w.wz * w.wa;
}

// out[a][p] = sum_b conj(Ai[b][a]) Aj[b][p] * I      (cpu/beams.py:129-145, 182-212;
// einsum "bas,s,bps->aps" in tests/test_cpu_beams.py:870)
__host__ __device__ inline void coh_AhB_flux(const cplx<double> Ai[4], const cplx<double> Aj[4],
                                             double I, cplx<double> o[4]) {
    for (int a = 0; a < 2; ++a)
        for (int p = 0; p < 2; ++p)
            o[a * 2 + p] = cscale(cadd(cmul(cconj(Ai[a]), Aj[p]), cmul(cconj(Ai[2 + a]), Aj[2 + p])), I);
}

// out[a][p] = sum_{b,k} conj(Ai[b][a]) C[b][k] Aj[k][p]   (cpu/beams.py:147-180, 215-246;
// einsum "bas,bks,kps->aps" in tests/test_cpu_beams.py:953)
__host__ __device__ inline void coh_AhCB(const cplx<double> Ai[4], const cplx<double> C[4],
                                         const cplx<double> Aj[4], cplx<double> o[4]) {
    for (int a = 0; a < 2; ++a) {
        const cplx<double> t0 = cadd(cmul(cconj(Ai[a]), C[0]), cmul(cconj(Ai[2 + a]), C[2]));
        const cplx<double> t1 = cadd(cmul(cconj(Ai[a]), C[1]), cmul(cconj(Ai[2 + a]), C[3]));
        for (int p = 0; p < 2; ++p) o[a * 2 + p] = cadd(cmul(t0, Aj[p]), cmul(t1, Aj[2 + p]));
    }
}

__host__ __device__ inline cplx<double> csqrt_principal(cplx<double> z) {
    const double r = hypot(z.re, z.im);
    if (r == 0.0) return {0.0, 0.0};
    double sr = sqrt(0.5 * (r + fabs(z.re)));
    double si = 0.5 * z.im / sr;
    if (z.re < 0) {  // swap so that the real part stays >= 0
        const double t = sr;
        sr = fabs(si);
        si = z.im < 0 ? -t : t;
    }
    return {sr, si};
}

// Stand-alone coherency op on reference-layout arrays (2, 2, n) [a][b][src]:
// variant 0: beam <- (A^H A) I          get_apparent_flux_polarized_beam   cpu/beams.py:129-145
//         1: beam <- A^H C A            get_apparent_flux_polarized        cpu/beams.py:147-180
//         2: out  <- Ai^H Aj I          ..._polarized_beam_pair            cpu/beams.py:182-212
//         3: out  <- Ai^H C Aj          ..._polarized_pair                 cpu/beams.py:215-246
//         4: out  <- sqrt(Bi Bj) I      unpolarized, (n) arrays            cpu_simulate.py:183-187
template <typename T>
__global__ void k_apparent_coherency(int variant, int64_t n, const cplx<T> *__restrict__ bi,
                                     const cplx<T> *__restrict__ bj, const void *__restrict__ flux,
                                     cplx<T> *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (variant == 4) {
        const cplx<double> a = {(double)bi[s].re, (double)bi[s].im}, b = {(double)bj[s].re, (double)bj[s].im};
        const cplx<double> r = cscale(csqrt_principal(cmul(a, b)), (double)((const T *)flux)[s]);
        out[s] = {(T)r.re, (T)r.im};
        return;
    }
    cplx<double> Ai[4], Aj[4], o[4];
    for (int i = 0; i < 4; ++i) {
        Ai[i] = {(double)bi[i * n + s].re, (double)bi[i * n + s].im};
        Aj[i] = {(double)bj[i * n + s].re, (double)bj[i * n + s].im};
    }
    if (variant == 0 || variant == 2) {
        coh_AhB_flux(Ai, Aj, (double)((const T *)flux)[s], o);
    } else {
        const cplx<T> *Cp = (const cplx<T> *)flux;
        cplx<double> C[4];
        for (int i = 0; i < 4; ++i) C[i] = {(double)Cp[i * n + s].re, (double)Cp[i * n + s].im};
        coh_AhCB(Ai, C, Aj, o);
    }
    for (int i = 0; i < 4; ++i) out[i * n + s] = {(T)o[i].re, (T)o[i].im};
}

// Stand-alone beam evaluation (GPUBeamEvaluator.evaluate_beam, gpu/beams.py:18-66):
// polarized -> (2, 2, n) [ax][feed][src]; else (n) power (imaginary part 0).
template <typename T, int ORD>
__global__ void k_beam_eval(BeamDesc b, int polarized, int fidx, double freq, int64_t n,
                            const T *__restrict__ az, const T *__restrict__ za,
                            cplx<T> *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (!polarized) {
        out[s] = {(T)eval_power<ORD>(b, fidx, freq, (double)az[s], (double)za[s]), T(0)};
        return;
    }
    cplx<double> A[4];
    eval_jones<ORD>(b, fidx, freq, (double)az[s], (double)za[s], A);
    for (int i = 0; i < 4; ++i) out[i * n + s] = {(T)A[i].re, (T)A[i].im};
}

// b[:, j] <- rot b[:, j]   (gpu/utils.py:8-22; cpu/utils.py:5-24)
template <typename T>
__global__ void k_inplace_rot(Rot9 r, T *__restrict__ b, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double x = b[j], y = b[n + j], z = b[2 * n + j];
    b[j] = (T)(r.m[0] * x + r.m[1] * y + r.m[2] * z);
    b[n + j] = (T)(r.m[3] * x + r.m[4] * y + r.m[5] * z);
    b[2 * n + j] = (T)(r.m[6] * x + r.m[7] * y + r.m[8] * z);
}

// ---------------------------------------------------------------------------------------------
// per-source astrometry from a per-time context (reference cpu_simulate.py:693-709,937)
// ---------------------------------------------------------------------------------------------
// ICRS -> observed is a source-independent context per time -- what ERFA keeps in eraASTROM and erfa.apco13 (or
// astropy's erfa_astrom) fills in microseconds on the host -- applied to every source: light deflection by the Sun,
// annual aberration, bias-precession-nutation (ICRS -> CIRS: the published algorithm of eraAtciqz = eraLdsun + eraAb +
// the BPN matrix), then Earth rotation, polar motion, diurnal aberration, the rotation to the local horizon and the
// A tan z + B tan^3 z refraction (CIRS -> observed: eraAtioq).  The context is taken in eraASTROM's field order so
// that a caller can hand over the bytes of the array ERFA filled.  One thread per source; arithmetic in fp64 whatever
// the catalog's precision.  Output: topocentric (east, north, up) unit vectors, the layout of fv_sim_set_topo.
// PARITY UNPINNED versus ERFA / matvis (neither is in this pipeline): pinned to the numpy restatement in oracle/.
struct Astrom {
    double pmt, eb[3], eh[3], em, v[3], bm1, bpn[9], along, phi, xpl, ypl, sphi, cphi, diurab, eral, refa, refb;
};
static_assert(sizeof(Astrom) == 31 * sizeof(double), "eraASTROM is 31 doubles");

__device__ inline void astrom_icrs_to_enu(const Astrom &a, double px, double py, double pz, double *enu) {
    constexpr double SRS = 1.97412574336e-8;  // Schwarzschild radius of the Sun in au
    // light deflection by the Sun (unit mass; q = p: the source is at infinity)
    const double em2 = fmax(a.em * a.em, 1.0), dlim = 1e-6 / em2;
    const double qdqpe = px * (px + a.eh[0]) + py * (py + a.eh[1]) + pz * (pz + a.eh[2]);
    const double wd = SRS / a.em / fmax(qdqpe, dlim);
    const double ex = a.eh[1] * pz - a.eh[2] * py, ey = a.eh[2] * px - a.eh[0] * pz, ez = a.eh[0] * py - a.eh[1] * px;  // e x q
    double qx = px + wd * (py * ez - pz * ey), qy = py + wd * (pz * ex - px * ez), qz = pz + wd * (px * ey - py * ex);  // p + w p x (e x q)
    // annual aberration (relativistic, with the Sun's potential term)
    const double pdv = qx * a.v[0] + qy * a.v[1] + qz * a.v[2];
    const double w1 = 1.0 + pdv / (1.0 + a.bm1), w2 = SRS / a.em;
    double ax = qx * a.bm1 + w1 * a.v[0] + w2 * (a.v[0] - pdv * qx);
    double ay = qy * a.bm1 + w1 * a.v[1] + w2 * (a.v[1] - pdv * qy);
    double az = qz * a.bm1 + w1 * a.v[2] + w2 * (a.v[2] - pdv * qz);
    const double rn = 1.0 / sqrt(ax * ax + ay * ay + az * az);
    ax *= rn;
    ay *= rn;
    az *= rn;
    // bias-precession-nutation: CIRS
    const double cx = a.bpn[0] * ax + a.bpn[1] * ay + a.bpn[2] * az;
    const double cy = a.bpn[3] * ax + a.bpn[4] * ay + a.bpn[5] * az;
    const double cz = a.bpn[6] * ax + a.bpn[7] * ay + a.bpn[8] * az;
    // Earth rotation: (-HA, Dec) Cartesian
    double se, ce;
    sincos(a.eral, &se, &ce);
    const double x = ce * cx + se * cy, y = -se * cx + ce * cy, z = cz;
    // polar motion
    double sx, cxp, sy, cyp;
    sincos(a.xpl, &sx, &cxp);
    sincos(a.ypl, &sy, &cyp);
    const double xhd = cxp * x + sx * z;
    const double yhd = sx * sy * x + cyp * y - cxp * sy * z;
    const double zhd = -sx * cyp * x + sy * y + cxp * cyp * z;
    // diurnal aberration
    const double f = 1.0 - a.diurab * yhd;
    const double xhdt = f * xhd, yhdt = f * (yhd + a.diurab), zhdt = f * zhd;
    // to the horizon frame (x south -> north is -x, y east, z up)
    const double xaet = a.sphi * xhdt - a.cphi * zhdt, yaet = yhdt, zaet = a.cphi * xhdt + a.sphi * zhdt;
    // refraction, A tan z + B tan^3 z with ERFA's guards near the horizon (identity for refa = refb = 0)
    double r = sqrt(xaet * xaet + yaet * yaet);
    r = r > 1e-6 ? r : 1e-6;
    const double zc = zaet > 0.05 ? zaet : 0.05;
    const double tz = r / zc, wr = a.refb * tz * tz;
    const double del = (a.refa + wr) * tz / (1.0 + (a.refa + 3.0 * wr) / (zc * zc));
    const double cosdel = 1.0 - del * del / 2.0, fr = cosdel - del * zc / r;
    const double xo = xaet * fr, yo = yaet * fr, zo = cosdel * zaet + del * r;
    const double on = 1.0 / sqrt(xo * xo + yo * yo + zo * zo);
    enu[0] = yo * on;
    enu[1] = -xo * on;
    enu[2] = zo * on;
}

// sources [off, off + n) of the (3, stride) catalog -> the same positions of a (3, stride) array of ENU vectors
template <typename T>
__global__ void k_astrom_topo(int64_t n, int64_t stride, int64_t off, const T *__restrict__ eq, Astrom a,
                              T *__restrict__ topo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = off + i;
    double enu[3];
    astrom_icrs_to_enu(a, (double)eq[j], (double)eq[stride + j], (double)eq[2 * stride + j], enu);
    topo[j] = (T)enu[0];
    topo[stride + j] = (T)enu[1];
    topo[2 * stride + j] = (T)enu[2];
}

struct StrengthArgs {
    int64_t M;          // capacity of the per-time arrays (stride); live count is *Mp
    int nfg;            // frequencies in this group
    int f_first;        // catalog index of the group's first frequency
    int nfreq;          // catalog frequency count (flux row length)
    int polarized, pol_sky, same_beam;
    int herm;           // strengths packed as two transforms (see k_interp): 1 Hermitian (c_00 + i c_11, c_01),
                        // 2 all real (c_00 + i c_11, c_01 + i c_10)
    int dim, w;
    double h[3], btc[3];
    int na[3];
    BeamDesc bi, bj;
    // height term k of a nearly flat array (Sim::run): strengths times ((z - wt_zc) wt_inv)^k, z = the sources' third
    // coordinate (compacted order).  A real factor: the Hermitian / all-real packings stay what they are.  wt_k <= 0: none.
    int wt_k;
    double wt_zc, wt_inv;
};

// Strengths of compacted source jc at catalog frequency fidx for one beam pair, times `pre`:
// tpol values written to dst.
template <typename T, int ORD>
__device__ inline void strength_eval(const StrengthArgs &a, int jc, int fidx, cplx<double> pre,
                                     const int *__restrict__ src_idx, const T *__restrict__ az,
                                     const T *__restrict__ za, const void *__restrict__ flux,
                                     const double *__restrict__ freqs, cplx<T> *__restrict__ dst) {
    const double freq = freqs[fidx];
    const int64_t js = src_idx[jc];   // catalog index
    const double azv = az[jc], zav = za[jc];
    if (!a.polarized) {
        // cpu_simulate.py:183-187: sqrt(B_i B_j) * I   (principal square root)
        const double bi = eval_power<ORD>(a.bi, fidx, freq, azv, zav);
        const double bj = a.same_beam ? bi : eval_power<ORD>(a.bj, fidx, freq, azv, zav);
        const double I = (double)((const T *)flux)[js * a.nfreq + fidx];
        cplx<double> c = cscale(csqrt_principal(cplx<double>{bi * bj, 0.0}), I);
        c = cmul(c, pre);
        dst[0] = {(T)c.re, (T)c.im};
        return;
    }
    cplx<double> Ai[4], Aj[4];
    eval_jones<ORD>(a.bi, fidx, freq, azv, zav, Ai);
    if (a.same_beam) {
        for (int i = 0; i < 4; ++i) Aj[i] = Ai[i];
    } else {
        eval_jones<ORD>(a.bj, fidx, freq, azv, zav, Aj);
    }
    cplx<double> o[4];
    if (!a.pol_sky) {
        const double I = (double)((const T *)flux)[js * a.nfreq + fidx];
        coh_AhB_flux(Ai, Aj, I, o);
    } else {
        // cpu_simulate.py:142-156: the kernels run on A' = flip(A, axis 0)
        const cplx<T> *Cp = (const cplx<T> *)flux + (js * a.nfreq + fidx) * 4;
        cplx<double> C[4];
        for (int i = 0; i < 4; ++i) C[i] = {(double)Cp[i].re, (double)Cp[i].im};
        const cplx<double> Fi[4] = {Ai[2], Ai[3], Ai[0], Ai[1]};
        const cplx<double> Fj[4] = {Aj[2], Aj[3], Aj[0], Aj[1]};
        coh_AhCB(Fi, C, Fj, o);
    }
    if (a.herm == 1) {  // same beam on both sides: o is Hermitian (o_00, o_11 real, o_10 = conj o_01); pre = 1
        dst[0] = {(T)o[0].re, (T)o[3].re};
        dst[1] = {(T)o[1].re, (T)o[1].im};
        return;
    }
    if (a.herm == 2) {  // real Jones matrices on both sides, unpolarized sky: all four products are real
        dst[0] = {(T)o[0].re, (T)o[3].re};
        dst[1] = {(T)o[1].re, (T)o[2].re};
        return;
    }
    for (int r = 0; r < 4; ++r) {
        const cplx<double> v = cmul(o[r], pre);
        dst[r] = {(T)v.re, (T)v.im};
    }
}

// thread <-> (sorted source p, frequency fgi); fgi fastest so a wave reads flux rows contiguously
// and writes its tpol strengths back to back:  cs[p][fgi * tpol + r].
template <typename T, int ORD>
__global__ void k_strengths(StrengthArgs a, const int *__restrict__ Mp, const int *__restrict__ perm,
                            const int *__restrict__ src_idx, const T *__restrict__ az,
                            const T *__restrict__ za, const void *__restrict__ flux,
                            const double *__restrict__ freqs, const int *__restrict__ i0s,
                            const T *__restrict__ fs, cplx<T> *__restrict__ cs, const T *__restrict__ zsrc) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= min((int64_t)*Mp, a.M) * a.nfg) return;
    const int64_t p = idx / a.nfg;
    const int fgi = (int)(idx % a.nfg);
    const int fidx = a.f_first + fgi;
    // type-3 pre-phase exp(i nu btc . x'), x' rebuilt from the sorted grid coordinates
    double dot = 0.0;
    for (int d = 0; d < a.dim; ++d) {
        const double pos = (double)i0s[(int64_t)d * a.M + p] - (double)fs[(int64_t)d * a.M + p];
        dot += a.btc[d] * (pos - 0.5 * a.na[d]) * a.h[d];
    }
    cplx<double> pre = {1.0, 0.0};
    if (dot != 0.0) sincos(freqs[fidx] * dot, &pre.im, &pre.re);
    const int tp = a.herm ? 2 : a.polarized ? 4 : 1;
    cplx<T> *dst = cs + (p * a.nfg + fgi) * tp;
    strength_eval<T, ORD>(a, perm[p], fidx, pre, src_idx, az, za, flux, freqs, dst);
    if (a.wt_k > 0) {  // uniform
        // T_k(t), t = (z - zc) / zh in [-1, 1]: the Chebyshev polynomial of term k (three-term recurrence)
        const double t = ((double)zsrc[perm[p]] - a.wt_zc) * a.wt_inv;
        double sc = t, prev = 1.0;
        for (int i = 1; i < a.wt_k; ++i) {
            const double nx = 2.0 * t * sc - prev;
            prev = sc;
            sc = nx;
        }
        for (int r = 0; r < tp; ++r) dst[r] = {(T)((double)dst[r].re * sc), (T)((double)dst[r].im * sc)};
    }
}

// Position adjoint (fv_sim_run_position_adjoint): k_strengths' thread mapping and strength_eval -- beams, coherency and
// pre-phase evaluated once per (source, channel) -- written as THREE strength sets, the values times the source's three
// coordinates x_d = 2 pi (R topo)_d (xyz: (3, M) in compacted order, absolute, not relative to the box centre; the third
// one also where the transforms are 2-D).  Set d starts d * set_stride elements after cs, each in k_strengths' layout.
// The factors are real: the Hermitian / all-real packings stay what they are.  With height terms the Chebyshev factor
// of term wt_k multiplies all three sets.
template <typename T, int ORD>
__global__ void k_strengths_moments(StrengthArgs a, const int *__restrict__ Mp, const int *__restrict__ perm,
                                    const int *__restrict__ src_idx, const T *__restrict__ az,
                                    const T *__restrict__ za, const void *__restrict__ flux,
                                    const double *__restrict__ freqs, const int *__restrict__ i0s,
                                    const T *__restrict__ fs, cplx<T> *__restrict__ cs, const T *__restrict__ xyz,
                                    int64_t set_stride) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= min((int64_t)*Mp, a.M) * a.nfg) return;
    const int64_t p = idx / a.nfg;
    const int fgi = (int)(idx % a.nfg);
    const int fidx = a.f_first + fgi;
    double dot = 0.0;
    for (int d = 0; d < a.dim; ++d) {
        const double pos = (double)i0s[(int64_t)d * a.M + p] - (double)fs[(int64_t)d * a.M + p];
        dot += a.btc[d] * (pos - 0.5 * a.na[d]) * a.h[d];
    }
    cplx<double> pre = {1.0, 0.0};
    if (dot != 0.0) sincos(freqs[fidx] * dot, &pre.im, &pre.re);
    const int tp = a.herm ? 2 : a.polarized ? 4 : 1;
    const int jc = perm[p];
    cplx<T> *dst = cs + (p * a.nfg + fgi) * tp;
    strength_eval<T, ORD>(a, jc, fidx, pre, src_idx, az, za, flux, freqs, dst);  // set 0 holds the plain values for now
    const double x0 = (double)xyz[jc], x1 = (double)xyz[a.M + jc], x2 = (double)xyz[2 * a.M + jc];
    double sc = 1.0;
    if (a.wt_k > 0) {  // uniform: T_k((z - zc) / zh), as in k_strengths
        const double t = (x2 - a.wt_zc) * a.wt_inv;
        double prev = 1.0;
        sc = t;
        for (int i = 1; i < a.wt_k; ++i) {
            const double nx = 2.0 * t * sc - prev;
            prev = sc;
            sc = nx;
        }
    }
    const double w0 = x0 * sc, w1 = x1 * sc, w2 = x2 * sc;
    for (int r = 0; r < tp; ++r) {
        const double re = (double)dst[r].re, im = (double)dst[r].im;
        dst[r] = {(T)(re * w0), (T)(im * w0)};
        dst[set_stride + r] = {(T)(re * w1), (T)(im * w1)};
        dst[2 * set_stride + r] = {(T)(re * w2), (T)(im * w2)};
    }
}

// Baseline gradient from the position pass's inner products S (k_interp<.., GRAD>): S is (3, nfa, nbls) complex fp64 per
// stream, S[d][f][k] = sum over times and products of conj(G) D'_d with D'_d the forward of the strengths times x_d.
// 16 lanes <-> baseline k: per component the lanes sum -nu_f Im S[d][f][k] over the block's channels (dealt over the
// lanes) and over the S buffers in lane order, a fixed butterfly combines them, and lane d < 3 adds row d of R^T / c
// applied to the three sums -- from the transforms' frame (R b / c, seconds) to metres in the frame of b -- into
// gbls[k][d] (fp64).  One owner per slot, no atomics: the bits do not depend on timing.
struct PosReduceArgs {
    const cplx<double> *S[4];
    int nl, nfa, f_base;
    int64_t nbls;
    double rt[9];  // R^T / c, row-major
};
constexpr int POS_GROUP = 16;
__global__ void k_posgrad_reduce(PosReduceArgs a, const double *__restrict__ freqs, double *__restrict__ gbls) {
    const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / POS_GROUP;
    const int lg = threadIdx.x & (POS_GROUP - 1);
    if (k >= a.nbls) return;  // (whole groups exit together)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t ds = (int64_t)a.nfa * a.nbls;  // slots between two components
    for (int f = lg; f < a.nfa; f += POS_GROUP) {
        const double nu = freqs[a.f_base + f];
        const int64_t slot = (int64_t)f * a.nbls + k;
        double i0 = 0.0, i1 = 0.0, i2 = 0.0;
        for (int li = 0; li < a.nl; ++li) {  // (nl <= 4, uniform; the pointer is picked without indexing the argument block)
            const cplx<double> *S = li == 0 ? a.S[0] : li == 1 ? a.S[1] : li == 2 ? a.S[2] : a.S[3];
            i0 += S[slot].im;
            i1 += S[slot + ds].im;
            i2 += S[slot + 2 * ds].im;
        }
        s0 -= nu * i0;
        s1 -= nu * i1;
        s2 -= nu * i2;
    }
    for (int off = POS_GROUP / 2; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
    }
    const double g0 = a.rt[0] * s0 + a.rt[1] * s1 + a.rt[2] * s2;
    const double g1 = a.rt[3] * s0 + a.rt[4] * s1 + a.rt[5] * s2;
    const double g2 = a.rt[6] * s0 + a.rt[7] * s1 + a.rt[8] * s2;
    if (lg < 3) gbls[3 * k + lg] += lg == 0 ? g0 : lg == 1 ? g1 : g2;
}

// ---------------------------------------------------------------------------------------------
// Adjoint (fv_sim_run_adjoint; DESIGN.md "Adjoint").  Per (time, frequency group, beam pair) the forward writes
//     out[k, r] = cj_k( sum_j c_jr exp(i nu s_k b_k . x_j) ),   s_k = -1 and cj_k = conj for a flipped baseline,
// so with H = cj_k(G) the transpose is a type-3 transform with the roles swapped:
//     Z_jr = sum_u q_ur exp(i (s_u b_u) . (nu x_j)),   q_ur = sum of conj(H_kr) over the baselines k of run u,
// sources at the pair's distinct sign-adjusted vectors, targets at the directions scaled per channel, and
//     Re <A F, G> = sum_j Re sum_r c_jr(F) Z_jr.
// ---------------------------------------------------------------------------------------------
struct AdjStrengthArgs {
    int64_t nu;           // runs of the pair's list (NUFFT sources)
    int nfg, tpol;
    int64_t g_f_stride;   // elements between two channels of the G block
    int64_t pol_off[4];   // output slot of product r (the forward's layout)
    int transpose_flipped;
};

// 16 lanes <-> (run u, channel fg), u fastest: q is (nfg tpol, nu) row-major, the layout Nufft3::load_strengths reads.
// The run's members are dealt over the 16 lanes (a redundant vector of HERA-350 has up to a few hundred) and the lanes'
// sums combined in a fixed butterfly: the result does not depend on timing.
constexpr int ADJ_GROUP = 16;
template <typename T>
__global__ void k_adj_strengths(AdjStrengthArgs a, const cplx<T> *__restrict__ g, const int *__restrict__ idx,
                                const signed char *__restrict__ flip, const int *__restrict__ ustart,
                                cplx<T> *__restrict__ q, int *__restrict__ err_nan) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ADJ_GROUP;
    const int lg = threadIdx.x & (ADJ_GROUP - 1);
    if (i >= a.nu * a.nfg) return;  // (whole groups exit together)
    const int64_t u = i % a.nu;
    const int fg = (int)(i / a.nu);
    const int64_t m0 = ustart ? ustart[u] : u, m1 = ustart ? ustart[u + 1] : u + 1;
    const cplx<T> *gf = g + (int64_t)fg * a.g_f_stride;
    double sr[4] = {0.0, 0.0, 0.0, 0.0}, si[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int64_t m = m0 + lg; m < m1; m += ADJ_GROUP) {  // the baselines that share this vector
        const int64_t k = idx ? idx[m] : m;
        const bool neg = flip && flip[m];
        for (int r = 0; r < a.tpol; ++r) {
            const int rt = a.transpose_flipped && neg && a.tpol == 4 ? (r & 1) * 2 + (r >> 1) : r;
            const cplx<T> v = gf[a.pol_off[rt] + k];
            bad += !(v.re == v.re && v.im == v.im);
            sr[r] += (double)v.re;                      // conj(H): G itself when flipped, conj(G) otherwise
            si[r] += neg ? (double)v.im : -(double)v.im;
        }
    }
    for (int r = 0; r < a.tpol; ++r)
        for (int off = ADJ_GROUP / 2; off > 0; off >>= 1) {
            sr[r] += __shfl_xor(sr[r], off, 64);
            si[r] += __shfl_xor(si[r], off, 64);
        }
    if (lg < a.tpol) {
        const int r = lg;
        double vr = sr[0], vi = si[0];
        for (int rr = 1; rr < 4; ++rr)
            if (r == rr) {
                vr = sr[rr];
                vi = si[rr];
            }
        q[((int64_t)fg * a.tpol + r) * a.nu + u] = {(T)vr, (T)vi};
    }
    if (bad) atomicAdd(err_nan, bad);
}

// Basis beams (fv_sim_run_basis_adjoint, flux pass): per (k <= l) term the forward's basis epilogue adds
//     V_b[r] += w1_b M_r(b),   V_b[rs] += w2_b X_r(b)  (k != l; rs the feed-transposed slot),
//     w1 = conj(C[a1,k]) C[a2,l],  w2 = conj(C[a1,l]) C[a2,k],   X_r(b) = M_r(b)  or (exact form)  conj(M_r(-b)),
// M_r the transform of the (k, l) strengths.  So every member of a run enters with its own weights:
//     q_ur  = sum_b conj(G_b[r]) w1_b  (+ conj(G_b[rs]) w2_b, reference form)       at the run's vector b_u,
//     q'_ur = sum_b G_b[rs] conj(w2_b)                                             at -b_u (exact form: mirror != 0),
// the mirrored sources following the nu plain ones.  Same fold and butterfly as k_adj_strengths.
struct AdjBasisArgs {
    int kk, ll, nbasis, ncoef_freq, f_first, mirror;
};
template <typename T>
__global__ void k_adj_strengths_basis(AdjStrengthArgs a, AdjBasisArgs ba, const cplx<T> *__restrict__ g,
                                      const int *__restrict__ idx, const int *__restrict__ ustart,
                                      const cplx<T> *__restrict__ coef, const int *__restrict__ ant1,
                                      const int *__restrict__ ant2, cplx<T> *__restrict__ q, int *__restrict__ err_nan) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ADJ_GROUP;
    const int lg = threadIdx.x & (ADJ_GROUP - 1);
    if (i >= a.nu * a.nfg) return;  // (whole groups exit together)
    const int64_t u = i % a.nu;
    const int fg = (int)(i / a.nu);
    const int f = ba.f_first + fg;
    const int64_t m0 = ustart ? ustart[u] : u, m1 = ustart ? ustart[u + 1] : u + 1;
    const cplx<T> *gf = g + (int64_t)fg * a.g_f_stride;
    const bool offd = ba.kk != ba.ll;
    double sr[4] = {0.0, 0.0, 0.0, 0.0}, si[4] = {0.0, 0.0, 0.0, 0.0};  // at b
    double tr[4] = {0.0, 0.0, 0.0, 0.0}, ti[4] = {0.0, 0.0, 0.0, 0.0};  // at -b
    int bad = 0;
    for (int64_t m = m0 + lg; m < m1; m += ADJ_GROUP) {  // the baselines that share this vector (basis lists: none flipped)
        const int64_t k = idx ? idx[m] : m;
        const int64_t cs1 = (int64_t)ant1[k] * ba.nbasis, cs2 = (int64_t)ant2[k] * ba.nbasis;
        const cplx<T> c1k = coef[(cs1 + ba.kk) * ba.ncoef_freq + f], c2l = coef[(cs2 + ba.ll) * ba.ncoef_freq + f];
        const cplx<double> w1 = cmul(cplx<double>{(double)c1k.re, -(double)c1k.im}, cplx<double>{(double)c2l.re, (double)c2l.im});
        cplx<double> w2 = {0.0, 0.0};
        if (offd) {
            const cplx<T> c1l = coef[(cs1 + ba.ll) * ba.ncoef_freq + f], c2k = coef[(cs2 + ba.kk) * ba.ncoef_freq + f];
            w2 = cmul(cplx<double>{(double)c1l.re, -(double)c1l.im}, cplx<double>{(double)c2k.re, (double)c2k.im});
        }
        for (int r = 0; r < 4; ++r) {
            const cplx<T> v = gf[a.pol_off[r] + k];
            bad += !(v.re == v.re && v.im == v.im);
            const cplx<double> x1 = cmul(cplx<double>{(double)v.re, -(double)v.im}, w1);
            sr[r] += x1.re;
            si[r] += x1.im;
            if (offd) {
                const cplx<T> vt = gf[a.pol_off[(r & 1) * 2 + (r >> 1)] + k];
                if (ba.mirror) {
                    const cplx<double> x2 = cmul(cplx<double>{(double)vt.re, (double)vt.im}, cplx<double>{w2.re, -w2.im});
                    tr[r] += x2.re;
                    ti[r] += x2.im;
                } else {
                    const cplx<double> x2 = cmul(cplx<double>{(double)vt.re, -(double)vt.im}, w2);
                    sr[r] += x2.re;
                    si[r] += x2.im;
                }
            }
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int off = ADJ_GROUP / 2; off > 0; off >>= 1) {
            sr[r] += __shfl_xor(sr[r], off, 64);
            si[r] += __shfl_xor(si[r], off, 64);
            tr[r] += __shfl_xor(tr[r], off, 64);
            ti[r] += __shfl_xor(ti[r], off, 64);
        }
    if (lg < 8) {
        const int r = lg & 3, side = lg >> 2;
        double vr = side ? tr[0] : sr[0], vi = side ? ti[0] : si[0];
        for (int rr = 1; rr < 4; ++rr)
            if (r == rr) {
                vr = side ? tr[rr] : sr[rr];
                vi = side ? ti[rr] : si[rr];
            }
        const int64_t np = a.nu * (ba.mirror ? 2 : 1);  // sources of the transform
        if (!side || ba.mirror) q[((int64_t)fg * 4 + r) * np + side * a.nu + u] = {(T)vr, (T)vi};
    }
    if (bad) atomicAdd(err_nan, bad);
}

// NaN entries of a visibility-shaped input, counted where k_adj_strengths counts them (a call that runs only the
// coefficient pass has no strengths kernel to meet them)
template <typename T>
__global__ void k_count_nan(const cplx<T> *__restrict__ g, int64_t n, int *__restrict__ err_nan) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx<T> v = g[i];
        bad += !(v.re == v.re && v.im == v.im);
    }
    if (bad) atomicAdd(err_nan, bad);
}

// Coefficient gradient from the inner products S (k_interp<.., GRAD>): one wave per (antenna a, basis index k, channel f),
//     gcoefs[a,k,f] += sum_{b: a1(b) = a} sum_l C[a2(b),l,f] S_kl(b)  +  sum_{b: a2(b) = a} sum_l C[a1(b),l,f] conj(S_lk(b)),
// over the antenna's baselines in the order of the host's list (csr: 2 b + role, role 1 = second antenna; an
// auto-correlation is in it twice), dealt over the 64 lanes; the S lanes are summed in lane order, the 64 partial sums
// in a fixed butterfly: no atomics, the bits do not depend on timing.
struct CoefReduceArgs {
    const cplx<double> *S[4];
    int nl, K, nfa, f_base, nfreq, nant;
    int64_t nbls;
};
template <typename T>
__global__ void k_coef_reduce(CoefReduceArgs a, const int *__restrict__ csr_start, const int *__restrict__ csr,
                              const int *__restrict__ ant1, const int *__restrict__ ant2, const cplx<T> *__restrict__ coef,
                              cplx<T> *__restrict__ out) {
    const int64_t item = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (item >= (int64_t)a.nant * a.K * a.nfa) return;  // (whole waves exit together)
    const int f = (int)(item % a.nfa);
    const int k = (int)((item / a.nfa) % a.K);
    const int an = (int)(item / ((int64_t)a.nfa * a.K));
    double ar = 0.0, ai = 0.0;
    for (int e = csr_start[an] + lane; e < csr_start[an + 1]; e += 64) {
        const int code = csr[e];
        const int64_t b = code >> 1;
        const bool second = code & 1;
        const int64_t other = second ? ant1[b] : ant2[b];
        for (int l = 0; l < a.K; ++l) {
            const int term = second ? l * a.K + k : k * a.K + l;
            const int64_t slot = ((int64_t)term * a.nfa + f) * a.nbls + b;
            double xr = 0.0, xi = 0.0;
            for (int li = 0; li < a.nl; ++li) {
                const cplx<double> v = a.S[li][slot];
                xr += v.re;
                xi += v.im;
            }
            if (second) xi = -xi;
            const cplx<T> c = coef[(other * a.K + l) * a.nfreq + a.f_base + f];
            ar += (double)c.re * xr - (double)c.im * xi;
            ai += (double)c.re * xi + (double)c.im * xr;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_xor(ar, off, 64);
        ai += __shfl_xor(ai, off, 64);
    }
    if (lane == 0) {
        cplx<T> *o = out + ((int64_t)an * a.K + k) * a.nfreq + a.f_base + f;
        *o = {(T)((double)o->re + ar), (T)((double)o->im + ai)};
    }
}

struct AdjAccArgs {
    int64_t M;           // capacity of the per-time arrays (stride of z); live count is *Mp
    int nfg, f_first;    // channels of the group, catalog index of its first
    int f_base, nfa;     // first channel of the run and channels the accumulator holds
    int polarized, pol_sky, same_beam;
    BeamDesc bi, bj;
};

// Transpose of strength_eval, thread <-> (compacted source jc, channel fg), jc fastest.  acc (fp64, this lane's) is
// (nsrc, nfa) for Stokes I skies, (nsrc, nfa, 2, 2) complex for coherency skies: the gradient with respect to the
// coherency, Re <A C, G> = Re sum conj(acc) C.  src_idx is injective within a slice: plain read-modify-write.
template <typename T, int ORD>
__global__ void k_adj_accumulate(AdjAccArgs a, const int *__restrict__ Mp, const int *__restrict__ src_idx,
                                 const T *__restrict__ az, const T *__restrict__ za, const double *__restrict__ freqs,
                                 const cplx<T> *__restrict__ z, double *__restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M * a.nfg) return;
    const int64_t jc = i % a.M;
    const int fg = (int)(i / a.M);
    if (jc >= (int64_t)*Mp) return;
    const int fidx = a.f_first + fg;
    const double freq = freqs[fidx];
    const int64_t js = src_idx[jc];
    const double azv = az[jc], zav = za[jc];
    const int tp = a.polarized ? 4 : 1;
    cplx<double> Z[4];
    for (int r = 0; r < tp; ++r) {
        const cplx<T> v = z[((int64_t)fg * tp + r) * a.M + jc];
        Z[r] = {(double)v.re, (double)v.im};
    }
    const int64_t slot = js * a.nfa + (fidx - a.f_base);
    if (!a.polarized) {  // c = sqrt(B_i B_j) I, principal root as in the forward
        const double bi = eval_power<ORD>(a.bi, fidx, freq, azv, zav);
        const double bj = a.same_beam ? bi : eval_power<ORD>(a.bj, fidx, freq, azv, zav);
        const cplx<double> beta = csqrt_principal(cplx<double>{bi * bj, 0.0});
        acc[slot] += beta.re * Z[0].re - beta.im * Z[0].im;
        return;
    }
    cplx<double> Ai[4], Aj[4];
    eval_jones<ORD>(a.bi, fidx, freq, azv, zav, Ai);
    if (a.same_beam) {
        for (int r = 0; r < 4; ++r) Aj[r] = Ai[r];
    } else {
        eval_jones<ORD>(a.bj, fidx, freq, azv, zav, Aj);
    }
    if (!a.pol_sky) {  // c_r = I (Ai^H Aj)_r
        cplx<double> o[4];
        coh_AhB_flux(Ai, Aj, 1.0, o);
        double s = 0.0;
        for (int r = 0; r < 4; ++r) s += o[r].re * Z[r].re - o[r].im * Z[r].im;
        acc[slot] += s;
        return;
    }
    // c_ap = sum_{b,k} conj(Fi[b][a]) C[b][k] Fj[k][p] on the flipped Jones F:  sum_ap c_ap Z_ap = sum_bk C_bk W_bk,
    // W_bk = sum_ap conj(Fi[b][a]) Fj[k][p] Z_ap;  the coherency gradient is conj(W)
    const cplx<double> Fi[4] = {Ai[2], Ai[3], Ai[0], Ai[1]};
    const cplx<double> Fj[4] = {Aj[2], Aj[3], Aj[0], Aj[1]};
    double *o = acc + slot * 8;
    for (int b = 0; b < 2; ++b)
        for (int k = 0; k < 2; ++k) {
            cplx<double> W = {0.0, 0.0};
            for (int a_ = 0; a_ < 2; ++a_)
                for (int p = 0; p < 2; ++p) W = cadd(W, cmul(cmul(cconj(Fi[b * 2 + a_]), Fj[k * 2 + p]), Z[a_ * 2 + p]));
            o[2 * (b * 2 + k)] += W.re;
            o[2 * (b * 2 + k) + 1] -= W.im;
        }
}

// The lanes' accumulators summed in lane order (bitwise reproducible for a given lane count) and added to gflux
// (nsrc, nfreq[, 2, 2]) in the run's precision, channels [f_base, f_base + nfa).
struct AdjReduceArgs {
    const double *acc[4];
    int nl, nfa, f_base, nfreq, comps;  // comps: reals per (source, channel), 1 or 8
    int64_t nsrc;
};
template <typename T>
__global__ void k_adj_reduce(AdjReduceArgs a, T *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.nsrc * a.nfa * a.comps) return;
    double s = 0.0;
    for (int l = 0; l < a.nl; ++l) s += a.acc[l][e];
    const int64_t js = e / ((int64_t)a.nfa * a.comps);
    const int64_t rem = e - js * a.nfa * a.comps;
    const int64_t o = (js * a.nfreq + a.f_base) * a.comps + rem;
    out[o] = (T)((double)out[o] + s);
}

// ---------------------------------------------------------------------------------------------
// Source adjoint (fv_sim_run_source_adjoint; DESIGN.md "Sources"): the gradient with respect to the sources' topocentric
// unit vectors n_j(t).  With the flux adjoint's Z (above), Re <V, G> = sum_t sum_j sum_f Re sum_r c_jr(n_j) Z_jr(x_j),
// x = 2 pi R n, and
//     dZ_jr / dx_d = i nu Z(d)_jr,   Z(d) the same transform of the strengths q_ur times the d-th coordinate of the run's
//                                    sign-adjusted vector (k_src_moments),
// so the gradient is a phase term, -nu Im sum_r c_jr Z(d)_jr in the transforms' frame, plus a beam term,
// Re sum_r (dc_jr / dn) Z_jr with Z held fixed.
// ---------------------------------------------------------------------------------------------
// q is (rows, nu) row-major (k_adj_strengths' layout); set 1 + d, set_stride elements further on, gets q times pos[d][u].
template <typename T>
__global__ void k_src_moments(int64_t nu, int64_t rows, int D, const T *__restrict__ pos, cplx<T> *__restrict__ q,
                              int64_t set_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nu * rows) return;
    const int64_t u = i % nu;
    const cplx<T> v = q[i];
    for (int d = 0; d < D; ++d) {
        const T b = pos[(int64_t)d * nu + u];
        q[(int64_t)(d + 1) * set_stride + i] = {v.re * b, v.im * b};
    }
}

// Angular step of the beam term's central differences [rad], per precision of the run (profiles/MEASUREMENTS.md "Source
// adjoint": the steps a decade either side measured against the exact reference).  The beams are evaluated in fp64 at
// either precision; only Z differs.
constexpr double SRC_BEAM_STEP_FP64 = 1e-6;
constexpr double SRC_BEAM_STEP_FP32 = 1e-6;
// Near the zenith az turns by h / sin(za) over the stencil and the difference's truncation grows with (h / sin za)^2 -- on
// a bilinear table 13 (h / sin za)^2 of the beam term, 1.5e-6 of a source's row at za = 3e-3 --, while a smaller step pays
// in the rounding of za = pi / 2 - asin(sqrt(1 - sin^2 za)), 1e-16 / (sin za . h).  So the step is at most this fraction of
// sin(za): it takes over below za = 1.1 degrees (profiles/MEASUREMENTS.md, "Table beams at every order": the fractions
// either side), and never falls below h / 1000 (a source within 2e-5 rad of the zenith has no usable az either way).
constexpr double SRC_BEAM_STEP_ZENITH = 5e-5;
__device__ inline double src_beam_step(double h, double e, double n) {
    return fmin(h, fmax(SRC_BEAM_STEP_ZENITH * sqrt(e * e + n * n), 1e-3 * h));
}

struct SrcAccArgs {
    int64_t M;           // capacity of the per-time arrays (stride of z); live count is *Mp
    int nfg, f_first;    // channels of the group, catalog index of its first
    int f_base, nfa;     // first channel of the block and channels the accumulator holds
    int nfreq;           // catalog frequency count (flux row length)
    int polarized, pol_sky, same_beam;
    int D;               // moment sets (2 on coplanar handles, 3 otherwise)
    int64_t set_stride;  // elements of z between two sets
    int64_t vstride;     // stride of vec (the catalog's source count)
    BeamDesc bi, bj;
    Rot9 rt;             // vec -> ENU at this time (identity for given topocentric vectors)
    Rot9 rp;             // the plane rotation R: ENU -> the transforms' frame
    double h;            // step of the beam term (src_beam_step shortens it near the zenith)
};

// A table at spline order 0 is piecewise constant: its derivative is exactly 0 wherever it exists, and a difference whose
// stencil straddles a jump returns (jump) / 2h, which is no derivative.  So with both beams of the pair such tables the
// beam term is 0 by definition and the displaced evaluations are skipped.  A dish paired with an order-0 table keeps the
// differences: the dish's factor varies smoothly (DESIGN.md "Sources": the limitation at a jump of that pair).
__device__ inline bool beam_term_is_zero(const SrcAccArgs &a) {
    return a.bi.kind == 1 && a.bi.order == 0 && (a.same_beam || (a.bj.kind == 1 && a.bj.order == 0));
}

// The forward's strengths of one source at the ENU unit vector (e, n, u), in fp64: strength_eval's beam and coherency
// calls (az, za as k_horizon_compact forms them) without its packings, pre-phase and rounding.  Returns
// s = Re sum_r c_r Z_r; c (tp values) is written when asked for.
template <typename T, int ORD>
__device__ inline double src_strength_dot(const SrcAccArgs &a, int fidx, double freq, int64_t js, double e, double n,
                                          const void *__restrict__ flux, const cplx<double> *Z, cplx<double> *c) {
    const double zeta = sqrt(fmax(0.0, 1.0 - (n * n + e * e)));
    double azv = fmod(0.5 * M_PI - atan2(e, n), 2.0 * M_PI);
    if (azv < 0) azv += 2.0 * M_PI;
    const double zav = 0.5 * M_PI - asin(zeta);
    if (!a.polarized) {
        const double bi = eval_power<ORD>(a.bi, fidx, freq, azv, zav);
        const double bj = a.same_beam ? bi : eval_power<ORD>(a.bj, fidx, freq, azv, zav);
        const double I = (double)((const T *)flux)[js * a.nfreq + fidx];
        const cplx<double> v = cscale(csqrt_principal(cplx<double>{bi * bj, 0.0}), I);
        if (c) c[0] = v;
        return v.re * Z[0].re - v.im * Z[0].im;
    }
    cplx<double> Ai[4], Aj[4], o[4];
    eval_jones<ORD>(a.bi, fidx, freq, azv, zav, Ai);
    if (a.same_beam) {
        for (int i = 0; i < 4; ++i) Aj[i] = Ai[i];
    } else {
        eval_jones<ORD>(a.bj, fidx, freq, azv, zav, Aj);
    }
    if (!a.pol_sky) {
        coh_AhB_flux(Ai, Aj, (double)((const T *)flux)[js * a.nfreq + fidx], o);
    } else {
        const cplx<T> *Cp = (const cplx<T> *)flux + (js * a.nfreq + fidx) * 4;
        cplx<double> C[4];
        for (int i = 0; i < 4; ++i) C[i] = {(double)Cp[i].re, (double)Cp[i].im};
        const cplx<double> Fi[4] = {Ai[2], Ai[3], Ai[0], Ai[1]};
        const cplx<double> Fj[4] = {Aj[2], Aj[3], Aj[0], Aj[1]};
        coh_AhCB(Fi, C, Fj, o);
    }
    double s = 0.0;
    for (int r = 0; r < 4; ++r) {
        if (c) c[r] = o[r];
        s += o[r].re * Z[r].re - o[r].im * Z[r].im;
    }
    return s;
}

// thread <-> (compacted source jc, channel fg), jc fastest, like k_adj_accumulate.  z holds 1 + D sets: Z, then Z(d).
// acc (fp64, this lane's) is (nsrc, nfa, 3): per (source, channel) the gradient in the transforms' frame, WITHOUT the
// factor 2 pi nu_f that k_srcgrad_reduce carries:
//     acc[d] += -Im sum_r c_r Z(d)_r  +  (R g_beam)_d / (2 pi nu),
// g_beam = D_1 e_1 + D_2 e_2 the tangential ENU gradient of s(n) = Re sum_r c_r(n) Z_r by central differences along the
// great circles through n towards an orthonormal tangent pair (e_1, e_2), n' = cos(h) n +- sin(h) e_i (R is a rotation:
// R^T, which the reduction applies, takes R g back to g).  The direction comes from the catalog vector in fp64, not
// from the lane's rounded az / za.  src_idx is injective within a slice: plain read-modify-write.
template <typename T, int ORD>
__global__ void k_src_accumulate(SrcAccArgs a, const int *__restrict__ Mp, const int *__restrict__ src_idx,
                                 const T *__restrict__ vec, const void *__restrict__ flux,
                                 const double *__restrict__ freqs, const cplx<T> *__restrict__ z,
                                 double *__restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M * a.nfg) return;
    const int64_t jc = i % a.M;
    const int fg = (int)(i / a.M);
    if (jc >= (int64_t)*Mp) return;
    const int fidx = a.f_first + fg;
    const double freq = freqs[fidx];
    const int64_t js = src_idx[jc];
    const int tp = a.polarized ? 4 : 1;
    double nv[3];
    {
        const double ex = vec[js], ey = vec[a.vstride + js], ez = vec[2 * a.vstride + js];
        nv[0] = a.rt.m[0] * ex + a.rt.m[1] * ey + a.rt.m[2] * ez;
        nv[1] = a.rt.m[3] * ex + a.rt.m[4] * ey + a.rt.m[5] * ez;
        nv[2] = a.rt.m[6] * ex + a.rt.m[7] * ey + a.rt.m[8] * ez;
        const double rn = 1.0 / sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
        for (int d = 0; d < 3; ++d) nv[d] *= rn;
    }
    cplx<double> Z[4], c[4];
    for (int r = 0; r < tp; ++r) {
        const cplx<T> v = z[((int64_t)fg * tp + r) * a.M + jc];
        Z[r] = {(double)v.re, (double)v.im};
    }
    src_strength_dot<T, ORD>(a, fidx, freq, js, nv[0], nv[1], flux, Z, c);
    // phase term
    double g[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < a.D; ++d) {
        const cplx<T> *zd = z + (int64_t)(d + 1) * a.set_stride;
        double s = 0.0;
        for (int r = 0; r < tp; ++r) {
            const cplx<T> v = zd[((int64_t)fg * tp + r) * a.M + jc];
            s += c[r].re * (double)v.im + c[r].im * (double)v.re;
        }
        if (d == 0) g[0] = -s;
        if (d == 1) g[1] = -s;
        if (d == 2) g[2] = -s;
    }
    // beam term: e_1 = n x (the axis n leans on least), normalised; e_2 = n x e_1
    double e1[3], e2[3];
    {
        const double a0 = fabs(nv[0]), a1 = fabs(nv[1]), a2 = fabs(nv[2]);
        if (a0 <= a1 && a0 <= a2) {
            e1[0] = 0.0, e1[1] = nv[2], e1[2] = -nv[1];
        } else if (a1 <= a2) {
            e1[0] = -nv[2], e1[1] = 0.0, e1[2] = nv[0];
        } else {
            e1[0] = nv[1], e1[1] = -nv[0], e1[2] = 0.0;
        }
        const double rn = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        for (int d = 0; d < 3; ++d) e1[d] *= rn;
        e2[0] = nv[1] * e1[2] - nv[2] * e1[1];
        e2[1] = nv[2] * e1[0] - nv[0] * e1[2];
        e2[2] = nv[0] * e1[1] - nv[1] * e1[0];
    }
    double sh, ch;
    const double h = src_beam_step(a.h, nv[0], nv[1]);
    sincos(h, &sh, &ch);
    const double inv2h = 0.5 / h;
    double d1 = 0.0, d2 = 0.0;
#pragma unroll 1
    for (int k = ORD == 0 && beam_term_is_zero(a) ? 4 : 0; k < 4; ++k) {  // +e_1, -e_1, +e_2, -e_2: one copy of the beam code
        const double sg = k & 1 ? -sh : sh;
        const double te = k < 2 ? e1[0] : e2[0], tn = k < 2 ? e1[1] : e2[1];
        const double s = src_strength_dot<T, ORD>(a, fidx, freq, js, ch * nv[0] + sg * te, ch * nv[1] + sg * tn, flux, Z, nullptr);
        const double w = k & 1 ? -inv2h : inv2h;
        if (k < 2) d1 += w * s;
        else d2 += w * s;
    }
    const double sc = 1.0 / (2.0 * M_PI * freq);
    const double b0 = d1 * e1[0] + d2 * e2[0], b1 = d1 * e1[1] + d2 * e2[1], b2 = d1 * e1[2] + d2 * e2[2];
    g[0] += sc * (a.rp.m[0] * b0 + a.rp.m[1] * b1 + a.rp.m[2] * b2);
    g[1] += sc * (a.rp.m[3] * b0 + a.rp.m[4] * b1 + a.rp.m[5] * b2);
    g[2] += sc * (a.rp.m[6] * b0 + a.rp.m[7] * b1 + a.rp.m[8] * b2);
    double *o = acc + (js * a.nfa + (fidx - a.f_base)) * 3;
    o[0] += g[0];
    o[1] += g[1];
    o[2] += g[2];
}

// One time step's accumulator -> its rows of gtopo (nsrc, 3) fp64, ENU: thread <-> catalog source j.  The channels of the
// block are summed in order with their factor nu_f, 2 pi R^T takes the sum from the transforms' frame to ENU, the radial
// component goes (the direction is a unit vector: only the tangential part means anything), and the row is added to.
// A time step belongs to one lane, so no sum runs over lanes: one owner per slot, no atomics, and the bits depend on
// neither timing nor FFTVIS_HIP_LANES.  A source below the horizon has an untouched accumulator and adds exactly 0.
struct SrcReduceArgs {
    int64_t nsrc;
    int nfa, f_base;
    Rot9 rt, rp;
};
template <typename T>
__global__ void k_srcgrad_reduce(SrcReduceArgs a, const double *__restrict__ acc, const T *__restrict__ vec,
                                 const double *__restrict__ freqs, double *__restrict__ gtopo) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.nsrc) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const double *p = acc + j * a.nfa * 3;
    for (int f = 0; f < a.nfa; ++f) {
        const double nu = freqs[a.f_base + f];
        s0 += nu * p[3 * f];
        s1 += nu * p[3 * f + 1];
        s2 += nu * p[3 * f + 2];
    }
    const double twopi = 2.0 * M_PI;
    double g0 = twopi * (a.rp.m[0] * s0 + a.rp.m[3] * s1 + a.rp.m[6] * s2);
    double g1 = twopi * (a.rp.m[1] * s0 + a.rp.m[4] * s1 + a.rp.m[7] * s2);
    double g2 = twopi * (a.rp.m[2] * s0 + a.rp.m[5] * s1 + a.rp.m[8] * s2);
    const double ex = vec[j], ey = vec[a.nsrc + j], ez = vec[2 * a.nsrc + j];
    double n0 = a.rt.m[0] * ex + a.rt.m[1] * ey + a.rt.m[2] * ez;
    double n1 = a.rt.m[3] * ex + a.rt.m[4] * ey + a.rt.m[5] * ez;
    double n2 = a.rt.m[6] * ex + a.rt.m[7] * ey + a.rt.m[8] * ez;
    if (!(n2 > 0.0)) return;  // below the horizon: the row stays what it is
    const double rn = 1.0 / sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    n0 *= rn, n1 *= rn, n2 *= rn;
    const double rad = g0 * n0 + g1 * n1 + g2 * n2;
    double *o = gtopo + 3 * j;
    o[0] += g0 - rad * n0;
    o[1] += g1 - rad * n1;
    o[2] += g2 - rad * n2;
}

// ---------------------------------------------------------------------------------------------
// Tangent (fv_sim_run_tangent; DESIGN.md "Tangents"), the source side: the change of the visibilities along a change
// delta_j = P_n dtopo_j of the sources' ENU unit vectors.  With out_k = cj_k( sum_j c_j(n_j) exp(i nu s_k b'_k . x_j) ),
// x = 2 pi R n,
//     d out_k = forward of dc_j  +  sum_d i nu b'_k,d (forward of c_j dx_j,d),    dx = 2 pi R delta,
// (a flipped baseline conjugates -i nu b' X into +i nu b' conj(X): no sign case), so the pass needs 1 + D strength sets.
// k_strengths' thread mapping (one thread per compacted source and channel); the sets are set_stride elements apart, each
// in k_strengths' layout, as k_strengths_moments writes its three:
//     set 0      dc = |delta| (c(n+) - c(n-)) / 2h,  n+- = cos(h) n +- sin(h) delta / |delta|: the beams' change along the
//                great circle through n towards delta, with c(n) evaluated in fp64 from the catalogue vector
//                (src_strength_dot's beam and coherency calls, two displaced evaluations), then brought into the
//                forward's form: pre-phase and Hermitian / all-real packing (the derivative of a Hermitian matrix along a
//                real direction is Hermitian, that of a real one real); exactly 0 where |delta| = 0 and between
//                order-0 tables (beam_term_is_zero);
//     set 1 + d  the forward's own strengths (strength_eval) times dx_d, d < D (2 on coplanar handles, where b'_z = 0).
// With height terms the Chebyshev factor of term wt_k multiplies every set.  s carries the beams and flags of a as
// src_strength_dot reads them, the rotations and the step.  dtopo: this time step's (nsrc, 3) fp64 rows, read at the
// compacted sources only -- a source below the horizon is in no list and its row is never read.
template <typename T, int ORD>
__global__ void k_strengths_tangent(StrengthArgs a, SrcAccArgs s, const int *__restrict__ Mp, const int *__restrict__ perm,
                                    const int *__restrict__ src_idx, const T *__restrict__ az,
                                    const T *__restrict__ za, const void *__restrict__ flux,
                                    const double *__restrict__ freqs, const int *__restrict__ i0s,
                                    const T *__restrict__ fs, cplx<T> *__restrict__ cs, const T *__restrict__ xyz,
                                    const T *__restrict__ vec, const double *__restrict__ dtopo) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= min((int64_t)*Mp, a.M) * a.nfg) return;
    const int64_t p = idx / a.nfg;
    const int fgi = (int)(idx % a.nfg);
    const int fidx = a.f_first + fgi;
    double dot = 0.0;
    for (int d = 0; d < a.dim; ++d) {
        const double pos = (double)i0s[(int64_t)d * a.M + p] - (double)fs[(int64_t)d * a.M + p];
        dot += a.btc[d] * (pos - 0.5 * a.na[d]) * a.h[d];
    }
    const double freq = freqs[fidx];
    cplx<double> pre = {1.0, 0.0};
    if (dot != 0.0) sincos(freq * dot, &pre.im, &pre.re);
    const int tp = a.herm ? 2 : a.polarized ? 4 : 1;
    const int jc = perm[p];
    const int64_t js = src_idx[jc];
    cplx<T> *dst = cs + (p * a.nfg + fgi) * tp;
    cplx<T> *d1 = dst + s.set_stride;
    strength_eval<T, ORD>(a, jc, fidx, pre, src_idx, az, za, flux, freqs, d1);  // set 1 holds the plain values for now
    double sc = 1.0;
    if (a.wt_k > 0) {  // uniform: T_k((z - zc) / zh), as in k_strengths
        const double t = ((double)xyz[2 * a.M + jc] - a.wt_zc) * a.wt_inv;
        double prev = 1.0;
        sc = t;
        for (int i = 1; i < a.wt_k; ++i) {
            const double nx = 2.0 * t * sc - prev;
            prev = sc;
            sc = nx;
        }
    }
    // n from the catalogue vector in fp64 (k_src_accumulate's), delta = P_n dtopo
    double nv[3], dl[3];
    {
        const double ex = vec[js], ey = vec[s.vstride + js], ez = vec[2 * s.vstride + js];
        nv[0] = s.rt.m[0] * ex + s.rt.m[1] * ey + s.rt.m[2] * ez;
        nv[1] = s.rt.m[3] * ex + s.rt.m[4] * ey + s.rt.m[5] * ez;
        nv[2] = s.rt.m[6] * ex + s.rt.m[7] * ey + s.rt.m[8] * ez;
        const double rn = 1.0 / sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
        for (int d = 0; d < 3; ++d) nv[d] *= rn;
        const double *dt = dtopo + 3 * js;
        const double rad = nv[0] * dt[0] + nv[1] * dt[1] + nv[2] * dt[2];
        for (int d = 0; d < 3; ++d) dl[d] = dt[d] - rad * nv[d];
    }
    const double twopi = 2.0 * M_PI;
    const double dx0 = twopi * (s.rp.m[0] * dl[0] + s.rp.m[1] * dl[1] + s.rp.m[2] * dl[2]) * sc;
    const double dx1 = twopi * (s.rp.m[3] * dl[0] + s.rp.m[4] * dl[1] + s.rp.m[5] * dl[2]) * sc;
    const double dx2 = twopi * (s.rp.m[6] * dl[0] + s.rp.m[7] * dl[1] + s.rp.m[8] * dl[2]) * sc;
    for (int r = 0; r < tp; ++r) {
        const double re = (double)d1[r].re, im = (double)d1[r].im;
        d1[r] = {(T)(re * dx0), (T)(im * dx0)};
        d1[s.set_stride + r] = {(T)(re * dx1), (T)(im * dx1)};
        if (s.D > 2) d1[2 * s.set_stride + r] = {(T)(re * dx2), (T)(im * dx2)};
    }
    // set 0: the beam term
    const double mag = sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
    cplx<double> dc[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    if (mag > 0.0 && !(ORD == 0 && beam_term_is_zero(s))) {
        double sh, ch;
        const double h = src_beam_step(s.h, nv[0], nv[1]);
        sincos(h, &sh, &ch);
        const double e0 = dl[0] / mag, e1 = dl[1] / mag;
        const double wgt = sc * mag * 0.5 / h;
        const cplx<double> Z[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {  // n+, n-: one copy of the beam code
            const double sg = k ? -sh : sh;
            cplx<double> c[4];
            src_strength_dot<T, ORD>(s, fidx, freq, js, ch * nv[0] + sg * e0, ch * nv[1] + sg * e1, flux, Z, c);
            const double w = k ? -wgt : wgt;
            for (int r = 0; r < (a.polarized ? 4 : 1); ++r) {
                dc[r].re += w * c[r].re;
                dc[r].im += w * c[r].im;
            }
        }
    }
    if (a.herm == 1) {  // Hermitian: dc_00, dc_11 real, dc_10 = conj dc_01; pre = 1
        dst[0] = {(T)dc[0].re, (T)dc[3].re};
        dst[1] = {(T)dc[1].re, (T)dc[1].im};
    } else if (a.herm == 2) {  // all four real
        dst[0] = {(T)dc[0].re, (T)dc[3].re};
        dst[1] = {(T)dc[1].re, (T)dc[2].re};
    } else {
        for (int r = 0; r < tp; ++r) {
            const cplx<double> v = cmul(dc[r], pre);
            dst[r] = {(T)v.re, (T)v.im};
        }
    }
}

// the same for a complex array of the handle's precision (fv_sim_run_basis_tangent's directions)
template <typename T>
__global__ void k_count_nonfinite_c(const cplx<T> *__restrict__ v, int64_t n, int *__restrict__ count) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad += isfinite(v[i].re) && isfinite(v[i].im) ? 0 : 1;
    if (bad) atomicAdd(count, bad);
}

// entries of a fp64 array that are not finite, added to *count (fv_sim_run_tangent's device-side inputs)
__global__ void k_count_nonfinite(const double *__restrict__ v, int64_t n, int *__restrict__ count) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad += isfinite(v[i]) ? 0 : 1;
    if (bad) atomicAdd(count, bad);
}

// ---------------------------------------------------------------------------------------------
// Type-1 path (lattice arrays): cpu_nufft2d_type1 (cpu/nufft.py:120-175), set-up
// cpu_simulate.py:661-681, per-slice :964-965,990-992,259-269.
// Visibility of the integer baseline (bx, by) at frequency nu is mode (bx, by) of a type-1
// transform of the sources at angles (tx, ty) = nu * 2 pi B^T topo.  Positions depend on nu, so
// every (source, frequency) pair becomes an entry of its own on that frequency's periodic
// n2 x n2 grid; entries whose footprint crosses the edge get periodic images.  Spread (same
// gather scheme as k_spread2d), pruned FFT keeping the n_modes central outputs, then modes are
// picked and deconvolved -- no gather at non-uniform targets at all.
// ---------------------------------------------------------------------------------------------
constexpr int T1_PAD = 16;  // origins run from -PAD .. n2: bins are offset by PAD cells

struct T1Args {
    int n2, nb1, w, nfg, f_first;
    int64_t cap;       // stride of xyz
    int64_t ecap;      // entry capacity
    int rec;           // bytes per entry record (multiple of 64)
};
// Entry record (rec bytes, 64-B aligned): {int i0x, i0y, ent, 0} then T wx[w], wy[w], zero padding.
// One record per (source, frequency[, periodic image]) in bin order: the scatter writes whole
// 64-B sectors (the earlier split arrays -- 72-B weight rows at arbitrary offsets -- cost 4x their
// size in WRITE_SIZE) and the spread stages a chunk of entries from one contiguous run.
constexpr int T1_HDR = 16;
inline int t1_record_bytes(int w, size_t real_bytes) {
    return (int)((T1_HDR + 2 * (size_t)w * real_bytes + 63) / 64 * 64);
}

// Footprint origin (and first kernel argument) of compacted source p at frequency f.
template <typename T>
__device__ inline void t1_origin(const T1Args &a, const T *__restrict__ xyz, int64_t p, double freq,
                                 int &i0x, int &i0y, double &fx, double &fy) {
    const double inv2pi = 0.5 / M_PI;
    double ux = (double)xyz[p] * freq * inv2pi, uy = (double)xyz[a.cap + p] * freq * inv2pi;
    ux -= floor(ux + 0.5);  // [-0.5, 0.5)
    uy -= floor(uy + 0.5);
    const double px = (ux + 0.5) * a.n2, py = (uy + 0.5) * a.n2;
    i0x = (int)ceil(px - 0.5 * a.w);
    i0y = (int)ceil(py - 0.5 * a.w);
    fx = (double)i0x - px;
    fy = (double)i0y - py;
}

// COUNT = true: histogram of entries per (frequency, bin); false: scatter + tabulate weights.
// W: the kernel width at compile time (9: the default tolerance in fp64; 0: any) -- with it the record is built
// in registers and leaves as 16-byte stores (12 for w = 9) instead of 2 w + padding scattered 8-byte ones.
// IMG = false (the type-2 adjoint's gather, k_t2_gather): one entry per (source, frequency) and no periodic images --
// the gather loads its tile with wrapped indices.
template <typename T, bool COUNT, int W = 0, bool IMG = true>
__global__ void k_t1_bin(T1Args a, const int *__restrict__ Mp, const T *__restrict__ xyz,
                         const double *__restrict__ freqs, int *__restrict__ counts,
                         const int *__restrict__ bin_start, int *__restrict__ cursor,
                         unsigned char *__restrict__ recs, T beta, T c4, int *__restrict__ overflow) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= min((int64_t)*Mp, a.cap) * a.nfg) return;
    const int64_t p = idx / a.nfg;
    const int f = (int)(idx % a.nfg);
    int i0x, i0y;
    double fx, fy;
    t1_origin<T>(a, xyz, p, freqs[a.f_first + f], i0x, i0y, fx, fy);
    // periodic images: every origin congruent mod n2 whose footprint reaches [0, n2)
    const int ox[2] = {0, !IMG ? 0 : i0x < 0 ? a.n2 : (i0x + a.w > a.n2 ? -a.n2 : 0)};
    const int oy[2] = {0, !IMG ? 0 : i0y < 0 ? a.n2 : (i0y + a.w > a.n2 ? -a.n2 : 0)};
    for (int iy = 0; iy < (oy[1] ? 2 : 1); ++iy)
        for (int ix = 0; ix < (ox[1] ? 2 : 1); ++ix) {
            const int jx = i0x + ox[ix], jy = i0y + oy[iy];
            const int bin = (f * a.nb1 + ((jy + T1_PAD) >> BINLOG)) * a.nb1 + ((jx + T1_PAD) >> BINLOG);
            if (COUNT) {
                atomicAdd(&counts[bin], 1);
            } else {
                const int64_t pos = bin_start[bin] + atomicAdd(&cursor[bin], 1);
                if (pos >= a.ecap) {
                    atomicAdd(overflow, 1);
                    continue;
                }
                unsigned char *rec = recs + pos * a.rec;
                *reinterpret_cast<int4 *>(rec) = make_int4(jx, jy, (int)idx, 0);  // ent = p * nfg + f
                T *wr = reinterpret_cast<T *>(rec + T1_HDR);
                if constexpr (W > 0) {
                    constexpr int PER = 16 / (int)sizeof(T);                       // reals per 16-byte store
                    constexpr int NV = (T1_HDR + 2 * W * (int)sizeof(T) + 63) / 64 * 64 / (int)sizeof(T) - T1_HDR / (int)sizeof(T);
                    T v[NV];
#pragma unroll
                    for (int k = 0; k < NV; ++k)
                        v[k] = k < W ? es_eval<T>((T)(fx + k), beta, c4) : k < 2 * W ? es_eval<T>((T)(fy + (k - W)), beta, c4) : T(0);
                    struct alignas(16) V16 { T x[PER]; };
#pragma unroll
                    for (int k = 0; k < NV; k += PER) {
                        V16 t;
#pragma unroll
                        for (int i = 0; i < PER; ++i) t.x[i] = v[k + i];
                        *reinterpret_cast<V16 *>(wr + k) = t;
                    }
                } else {
                    const int nreal = (a.rec - T1_HDR) / (int)sizeof(T);
                    for (int k = 0; k < a.w; ++k) wr[k] = es_eval<T>((T)(fx + k), beta, c4);
                    for (int k = 0; k < a.w; ++k) wr[a.w + k] = es_eval<T>((T)(fy + k), beta, c4);
                    for (int k = 2 * a.w; k < nreal; ++k) wr[k] = T(0);  // whole sectors, no partial writes
                }
            }
        }
}

template <typename T, int ORD>
__global__ void k_t1_strengths(StrengthArgs a, const int *__restrict__ nent, int64_t ecap,
                               const unsigned char *__restrict__ recs, int rec, const int *__restrict__ src_idx,
                               const T *__restrict__ az, const T *__restrict__ za,
                               const void *__restrict__ flux, const double *__restrict__ freqs,
                               cplx<T> *__restrict__ cs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= min((int64_t)*nent, ecap)) return;  // entries beyond the capacity were dropped (and flagged) by k_t1_bin
    const int id = reinterpret_cast<const int *>(recs + e * rec)[2];
    const int tp = a.herm ? 2 : a.polarized ? 4 : 1;
    strength_eval<T, ORD>(a, id / a.nfg, a.f_first + id % a.nfg, cplx<double>{1.0, 0.0}, src_idx, az, za,
                     flux, freqs, cs + e * tp);
}

// One wave per 16 x 16 cell tile of one frequency plane (lane = (x, y): cells (x | x + 8, y | y + 8)); TP =
// transforms per plane (1, 2 or 4).  The wave walks the entries of the 3 x 3 bins whose footprints reach the tile in
// chunks of 16 -- 0.42 entry visits per cell instead of the 0.75 of an 8 x 8 block per wave:
//   * the origin of an entry is wave-uniform: lane j of the chunk loads entry j's header and the loop over the
//     entries pulls it into scalar registers with v_readlane; the TP strengths are read back from LDS by every
//     lane (a broadcast: LDS returns bytes per lane whether or not the address is shared), which for four cells
//     per lane is a quarter of the LDS bytes per cell of the one-cell version (that one was LDS-bound at 0.14 of
//     HBM peak; all-readlane strengths made an 8 x 16 version VALU-bound instead: 10 readlanes per entry).
//   * only the 2 w kernel weights go through LDS, rows of w + 2 values with a zero at either end: a lane clamps its
//     offsets into [-1, w] (one v_med3 each) instead of testing them, and reads x, y and y + 8.
// Every cell of the plane is written exactly once; no atomics.
template <typename T, int TP>
__global__ __launch_bounds__(SPREAD_THREADS) void k_t1_spread(
    T1Args a, const unsigned char *__restrict__ recs, const int *__restrict__ bin_start,
    const cplx<T> *__restrict__ cs, cplx<T> *__restrict__ grid) {
    constexpr int KW = MAX_W + 2;
    constexpr int TL = BINLOG + 1;  // tile = 16 x 16 cells
    __shared__ T s_kw[SPREAD_THREADS / 64][SPREAD_CHUNK][2][KW];
    __shared__ cplx<T> s_str[SPREAD_THREADS / 64][SPREAD_CHUNK][TP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int bx2 = blockIdx.x * 4 + wave, by2 = blockIdx.y, f = blockIdx.z;
    if (bx2 >= (a.n2 >> TL)) return;  // wave-uniform; the waves of a workgroup share nothing
    const int tx0 = bx2 << TL, ty0 = by2 << TL;  // the tile's first cell (uniform)
    const int cx = tx0 + (lane & 7), cy = ty0 + (lane >> 3);
    T ar[4][TP], ai[4][TP];  // cells (cx, cy), (cx + 8, cy), (cx, cy + 8), (cx + 8, cy + 8)
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int q = 0; q < TP; ++q) ar[h][q] = ai[h][q] = T(0);
    const int w = a.w;
    // zero guards of the weight rows (slots 0 and w + 1), written once
    for (int e = lane; e < SPREAD_CHUNK * 4; e += 64) s_kw[wave][e >> 2][(e >> 1) & 1][(e & 1) ? w + 1 : 0] = T(0);
    const int bxl = ((bx2 << TL) - w + 1 + T1_PAD) >> BINLOG, bxh = ((bx2 << TL) + 15 + T1_PAD) >> BINLOG;
    const int byl = ((by2 << TL) - w + 1 + T1_PAD) >> BINLOG, byh = ((by2 << TL) + 15 + T1_PAD) >> BINLOG;
    // The chunks of the <= 3 bin rows form one sequence; chunk c + 1 is requested (global -> registers) before chunk
    // c is accumulated, so its loads fly under the accumulation.
    constexpr int NWV = (2 * MAX_W + 3) / 4;  // weights per staging lane (4 lanes per entry)
    int yb = byl, s1 = 0, base = 0;
    auto open_row = [&]() {  // [base, s1) of bin row yb; (entries beyond the capacity were dropped and flagged by k_t1_bin)
        const int rowb = (f * a.nb1 + yb) * a.nb1;
        base = __builtin_amdgcn_readfirstlane(bin_start[rowb + bxl]);
        s1 = __builtin_amdgcn_readfirstlane((int)min((int64_t)bin_start[rowb + bxh + 1], a.ecap));
    };
    auto next_chunk = [&](int &cb, int &cn) {  // false: no chunk left
        while (base >= s1) {
            if (yb > byh) return false;
            open_row();
            ++yb;
        }
        cb = base;
        cn = min(SPREAD_CHUNK, s1 - base);
        base += cn;
        return true;
    };
    int2 hdr_n = make_int2(0, 0);
    cplx<T> sv_n = {T(0), T(0)};
    T wv_n[NWV];
    auto request = [&](int cb, int cn) {
        const unsigned char *rb = recs + (int64_t)cb * a.rec;
        if (lane < cn) hdr_n = *reinterpret_cast<const int2 *>(rb + (int64_t)lane * a.rec);
        if (lane < cn * TP) sv_n = cs[(int64_t)cb * TP + lane];
        const int j = lane >> 2;  // weights: 4 lanes per entry, every fourth value each
        const T *wr = reinterpret_cast<const T *>(rb + (int64_t)j * a.rec + T1_HDR);
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int k = (lane & 3) + 4 * i;
            wv_n[i] = j < cn && k < 2 * w ? wr[k] : T(0);
        }
    };
    int cb = 0, cn = 0;
    bool have = next_chunk(cb, cn);
    if (have) request(cb, cn);
    while (have) {
        const int n = cn;
        const int2 hdr = hdr_n;  // staging register: lane j = entry j's origin
        if (lane < n * TP) s_str[wave][lane / TP][lane % TP] = sv_n;
        {
            const int j = lane >> 2;
#pragma unroll
            for (int i = 0; i < NWV; ++i) {
                const int k = (lane & 3) + 4 * i;
                if (j < n && k < 2 * w) s_kw[wave][j][k >= w][(k >= w ? k - w : k) + 1] = wv_n[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        have = next_chunk(cb, cn);
        if (have) request(cb, cn);
        for (int j = 0; j < n; ++j) {
            const int ox = __builtin_amdgcn_readlane(hdr.x, j), oy = __builtin_amdgcn_readlane(hdr.y, j);
            // (Skipping, with scalar branches on the wave-uniform origin, the quadrants a footprint misses -- 1.8 of 4 are met
            // on average -- was measured slower: 1.63 against 1.22 ms per C3 time step; the branches break the schedule.)
            // offsets clamped into [-1, w]: the guards at either end of a row are zero
            const int dx = cx - ox, dy = cy - oy;
            auto clamp = [&](int v) {  // median(v, -1, w): one instruction (the compiler cannot prove -1 <= w for min(max()))
                int r;
                asm("v_med3_i32 %0, %1, -1, %2" : "=v"(r) : "v"(v), "s"(w));
                return r + 1;
            };
            const T wx0 = s_kw[wave][j][0][clamp(dx)], wx1 = s_kw[wave][j][0][clamp(dx + 8)];
            const T wy0 = s_kw[wave][j][1][clamp(dy)], wy1 = s_kw[wave][j][1][clamp(dy + 8)];
            const T wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
            for (int q = 0; q < TP; ++q) {
                const cplx<T> cv = s_str[wave][j][q];  // broadcast read
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    ar[h][q] += cv.re * wt[h];
                    ai[h][q] += cv.im * wt[h];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the rows are rewritten by the next chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int64_t plane = (int64_t)a.n2 * a.n2;
    cplx<T> *o = grid + (int64_t)f * TP * plane + (int64_t)cy * a.n2 + cx;
#pragma unroll
    for (int q = 0; q < TP; ++q)
#pragma unroll
        for (int h = 0; h < 4; ++h) o[q * plane + (int64_t)(h >> 1) * 8 * a.n2 + (h & 1) * 8] = {ar[h][q], ai[h][q]};
}

// The same tile walk with the accumulation on the matrix pipe (fp64).  A footprint's weights are separable, so the update
// of one 16 x 16 tile by the entries e that reach it is a matrix product per real component c of the strengths,
//     G_c[y][x] += sum_e (s_{e,c} wy_e[y]) wx_e[x]      --   A[y][e] = s_{e,c} wy_e[y] (16 x 4),  B[e][x] = wx_e[x] (4 x 16),
// v_mfma_f64_16x16x4_f64: four entries per instruction, 2 TP instructions (the real and imaginary parts of the TP
// transforms) per four entries.  fp64 MFMA has the vector pipe's flop rate on gfx950, and seven eighths of the products
// are by the zero guards here too; what it removes is everything around the multiply-adds -- the vector version spends 38
// instructions per (entry, tile) visit, 16 of them multiply-adds; here a visit is one MFMA (64 cycles) plus a quarter of
// two LDS reads, two clamps and 2 TP multiplies, issued beside it.  C3 lattice path: 1.22 -> see profiles/MEASUREMENTS.md.
// Operand layout (as k_spread2d_mm): lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15], r < 4.
// (The waves-per-SIMD bound is what makes the compiler keep the accumulators in vector registers: without it they
// travel to accumulator registers and back around every group of MFMAs -- 64 moves per four instructions, and moves
// issue on the same pipe: 25 vector instructions per MFMA, the kernel no faster than the vector version.)
template <int TP>
__global__ __launch_bounds__(SPREAD_THREADS, 4) void k_t1_spread_mm(
    T1Args a, const unsigned char *__restrict__ recs, const int *__restrict__ bin_start,
    const cplx<double> *__restrict__ cs, cplx<double> *__restrict__ grid) {
    using T = double;
    using d4 = double __attribute__((ext_vector_type(4)));
    constexpr int KW = MAX_W + 2;
    constexpr int TL = BINLOG + 1;  // tile = 16 x 16 cells
    __shared__ T s_kw[SPREAD_THREADS / 64][SPREAD_CHUNK][2][KW];
    __shared__ cplx<T> s_str[SPREAD_THREADS / 64][SPREAD_CHUNK][TP];
    __shared__ int s_org[SPREAD_THREADS / 64][SPREAD_CHUNK][2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int bx2 = blockIdx.x * 4 + wave, by2 = blockIdx.y, f = blockIdx.z;
    if (bx2 >= (a.n2 >> TL)) return;  // wave-uniform; the waves of a workgroup share nothing
    const int tx0 = bx2 << TL, ty0 = by2 << TL;
    const int li = lane & 15, g = lane >> 4;  // operand row / column, and the entry of a group of four
    d4 acc[2 * TP];
#pragma unroll
    for (int c = 0; c < 2 * TP; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    const int w = a.w;
    // zero guards of the weight rows (slots 0 and w + 1) and zero strengths / origins everywhere: the slots a short chunk
    // leaves untouched enter the products with zero strengths and finite weights
    for (int e = lane; e < SPREAD_CHUNK * 2 * KW; e += 64) (&s_kw[wave][0][0][0])[e] = T(0);
    for (int e = lane; e < SPREAD_CHUNK * TP; e += 64) (&s_str[wave][0][0])[e] = {T(0), T(0)};
    if (lane < SPREAD_CHUNK * 2) (&s_org[wave][0][0])[lane] = 0;
    const int bxl = (tx0 - w + 1 + T1_PAD) >> BINLOG, bxh = (tx0 + 15 + T1_PAD) >> BINLOG;
    const int byl = (ty0 - w + 1 + T1_PAD) >> BINLOG, byh = (ty0 + 15 + T1_PAD) >> BINLOG;
    constexpr int NWV = (2 * MAX_W + 3) / 4;  // weights per staging lane (4 lanes per entry)
    int yb = byl, s1 = 0, base = 0;
    auto open_row = [&]() {
        const int rowb = (f * a.nb1 + yb) * a.nb1;
        base = __builtin_amdgcn_readfirstlane(bin_start[rowb + bxl]);
        s1 = __builtin_amdgcn_readfirstlane((int)min((int64_t)bin_start[rowb + bxh + 1], a.ecap));
    };
    auto next_chunk = [&](int &cb, int &cn) {
        while (base >= s1) {
            if (yb > byh) return false;
            open_row();
            ++yb;
        }
        cb = base;
        cn = min(SPREAD_CHUNK, s1 - base);
        base += cn;
        return true;
    };
    int2 hdr_n = make_int2(0, 0);
    cplx<T> sv_n = {T(0), T(0)};
    T wv_n[NWV];
    // (every load is unconditional -- indices clamped into the chunk, the value selected afterwards: as conditional loads
    // each sat in an exec-masked region of its own with a branch around it, and vector instructions of the staging
    // serialise with the MFMAs on the SIMD)
    const int nwv = (2 * w + 3) >> 2;  // uniform
    auto request = [&](int cb, int cn) {  // cn >= 1
        const unsigned char *rb = recs + (int64_t)cb * a.rec;
        hdr_n = *reinterpret_cast<const int2 *>(rb + (int64_t)min(lane, cn - 1) * a.rec);
        sv_n = cs[(int64_t)cb * TP + min(lane, cn * TP - 1)];
        const int j = lane >> 2;
        const T *wr = reinterpret_cast<const T *>(rb + (int64_t)min(j, cn - 1) * a.rec + T1_HDR);
#pragma unroll
        for (int i = 0; i < NWV; ++i) {
            const int k = (lane & 3) + 4 * i;
            if (i < nwv) wv_n[i] = wr[min(k, 2 * w - 1)];  // uniform; used (or not) when the chunk is staged, not here
        }
    };
    int cb = 0, cn = 0;
    bool have = next_chunk(cb, cn);
    if (have) request(cb, cn);
    while (have) {
        const int n = cn;
        if (lane < SPREAD_CHUNK * TP) s_str[wave][lane / TP][lane % TP] = lane < n * TP ? sv_n : cplx<T>{T(0), T(0)};  // zero beyond the chunk's count
        if (lane < n) {
            s_org[wave][lane][0] = hdr_n.x - tx0;  // origin relative to the tile
            s_org[wave][lane][1] = hdr_n.y - ty0;
        }
        {
            const int j = lane >> 2;
#pragma unroll
            for (int i = 0; i < NWV; ++i) {
                const int k = (lane & 3) + 4 * i;
                if (j < n && k < 2 * w) s_kw[wave][j][k >= w][(k >= w ? k - w : k) + 1] = wv_n[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        have = next_chunk(cb, cn);
        if (have) request(cb, cn);
        auto clamp = [&](int v) {  // median(v, -1, w) + 1: the guards at either end of a row are zero
            int r;
            asm("v_med3_i32 %0, %1, -1, %2" : "=v"(r) : "v"(v), "s"(w));
            return r + 1;
        };
        const int nq = (n + 3) >> 2;
        for (int q = 0; q < nq; ++q) {
            const int e = 4 * q + g;  // this lane's entry (slots beyond n: zero strengths)
            const int ox = s_org[wave][e][0], oy = s_org[wave][e][1];
            const T wy = s_kw[wave][e][1][clamp(li - oy)];  // A: row y = li
            const T wx = s_kw[wave][e][0][clamp(li - ox)];  // B: column x = li
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                const cplx<T> sv = s_str[wave][e][t];
                acc[2 * t] = __builtin_amdgcn_mfma_f64_16x16x4f64(sv.re * wy, wx, acc[2 * t], 0, 0, 0);
                acc[2 * t + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(sv.im * wy, wx, acc[2 * t + 1], 0, 0, 0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the rows are rewritten by the next chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // results: lane l, register r = cell (x = tx0 + (l & 15), y = ty0 + (l >> 4) + 4 r): 16 lanes write 256 contiguous bytes
    const int64_t plane = (int64_t)a.n2 * a.n2;
    cplx<T> *o = grid + (int64_t)f * TP * plane + (int64_t)(ty0 + g) * a.n2 + tx0 + li;
#pragma unroll
    for (int t = 0; t < TP; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[t * plane + (int64_t)(4 * r) * a.n2] = {acc[2 * t][r], acc[2 * t + 1][r]};
}

// vis[f][pol][k] = X_{f,pol}[bx_k][by_k] / (psi_hat(bx) psi_hat(by)); flipped baselines take the
// negated mode and are conjugated (cpu_simulate.py:259,298).  X is stored [plane][lx][ly].
template <typename T>
__global__ void k_t1_pick(const cplx<T> *__restrict__ X, int no, int P, int cnt, int nfg, int tp,
                          const int *__restrict__ blx, const int *__restrict__ bly, int64_t N,
                          const int *__restrict__ bl_idx, const signed char *__restrict__ flip,
                          const T *__restrict__ dec, cplx<T> *__restrict__ out,
                          int64_t out_fg_stride, int64_t p0, int64_t p1, int64_t p2, int64_t p3, bool accumulate,
                          bool herm, bool tflip) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * nfg) return;
    const int f = (int)(idx / N);
    const int64_t kl = idx % N;
    const int64_t k = bl_idx ? bl_idx[kl] : kl;
    const bool fl = flip && flip[kl];
    const int mx = fl ? -blx[k] : blx[k], my = fl ? -bly[k] : bly[k];
    const int lx = mx + no / 2, ly = my + no / 2;
    const T d = dec[lx] * dec[ly];
    // tflip (reference_compat = 0): a flipped baseline's block goes to the feed-transposed slots (V_ij(-b)^H)
    const bool sw = fl && tflip && tp != 1;
    const int64_t pol[4] = {p0, sw ? p2 : p1, sw ? p1 : p2, p3};
    if (herm) {
        // Hermitian packing (see k_interp): planes T1 = F[c_00 + i c_11], T2 = F[c_01]; the mirror mode
        // (-mx, -my) is on the grid too and shares the deconvolution factor (psi_hat is even)
        const int lxm = -mx + no / 2, lym = -my + no / 2;
        const int64_t rows = (int64_t)P * cnt;
        const cplx<T> *X1 = X + ((int64_t)f * 2) * rows * no, *X2 = X1 + rows * no;
        const cplx<T> Pp = X1[(int64_t)out_pos(lx, P, cnt) * no + ly], Mm = X1[(int64_t)out_pos(lxm, P, cnt) * no + lym];
        const cplx<T> C = X2[(int64_t)out_pos(lx, P, cnt) * no + ly], D = X2[(int64_t)out_pos(lxm, P, cnt) * no + lym];
        const T h = T(0.5) * d;
        cplx<T> v[4];
        v[0] = {h * (Pp.re + Mm.re), h * (Pp.im - Mm.im)};   // (P + conj M) / 2
        v[3] = {h * (Pp.im + Mm.im), -h * (Pp.re - Mm.re)};  // (P - conj M) / 2i
        v[1] = {d * C.re, d * C.im};
        v[2] = {d * D.re, -d * D.im};                        // conj D
        for (int r = 0; r < 4; ++r) {
            if (fl) v[r].im = -v[r].im;
            cplx<T> &o = out[(int64_t)f * out_fg_stride + pol[r] + k];
            o = accumulate ? cplx<T>{o.re + v[r].re, o.im + v[r].im} : v[r];
        }
        return;
    }
    for (int r = 0; r < tp; ++r) {
        // rows (lx) are stored residue-major (DimGeom::out_pos), the contiguous ly in natural order
        cplx<T> v = X[(((int64_t)f * tp + r) * ((int64_t)P * cnt) + out_pos(lx, P, cnt)) * no + ly];
        v = {v.re * d, fl ? -v.im * d : v.im * d};
        cplx<T> &o = out[(int64_t)f * out_fg_stride + pol[r] + k];
        o = accumulate ? cplx<T>{o.re + v.re, o.im + v.im} : v;
    }
}

// ---------------------------------------------------------------------------------------------
// Type-2 adjoint of the type-1 path (Sim::adjoint_flux_type2; DESIGN.md "Adjoint").  The transpose of the slice above:
//     Z_jr = sum_m q_mr exp(+i m . theta_j),   q_mr = sum of conj(H_kr) over the baselines at (sign-adjusted) mode m,
// H the flip-adjusted conj(G) of k_adj_strengths.  Mode fill (deconvolved, exact zeros elsewhere), the pruned FFT the
// other way round (na = n_modes + 1 inputs, all n2 outputs), periodic gather at the (source, frequency) entries.
// ---------------------------------------------------------------------------------------------

// Thread <-> (cell ix fastest, iy, plane = (channel, product)) of the FFT's input planes A [plane][iy][ix], mode =
// index - na / 2.  cell_start / cell_runs: the runs (k_adj_strengths' u) at each cell of ONE plane -- one run for a
// pair's list in (u, v) order, every member of its own when the list was left as given; summed in list order.  Every
// cell is written once: no memset, no atomics.
template <typename T>
__global__ void k_t2_fill(int na, int nplanes, int64_t nu, const int *__restrict__ cell_start,
                          const int *__restrict__ cell_runs, const cplx<T> *__restrict__ q, const T *__restrict__ dec,
                          cplx<T> *__restrict__ A) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t cells = (int64_t)na * na;
    if (idx >= cells * nplanes) return;
    const int c = (int)(idx % cells);
    const int64_t plane = idx / cells;
    const int ix = c % na, iy = c / na;
    double sr = 0.0, si = 0.0;
    for (int k = cell_start[c]; k < cell_start[c + 1]; ++k) {
        const cplx<T> v = q[plane * nu + cell_runs[k]];
        sr += (double)v.re;
        si += (double)v.im;
    }
    const double d = (double)dec[ix] * (double)dec[iy];
    A[idx] = {(T)(sr * d), (T)(si * d)};
}

// One workgroup of four waves per (frequency, 8 x 8-cell bin of footprint origins) of k_t1_bin<.., IMG = false>'s
// entry order; TP = transforms per plane (1 or 4).  The bin's entries all read one (8 + w - 1)^2 tile of the
// transform's output X [plane][out_pos(lx)][ly]: the workgroup stages it in LDS once, with wrapped indices (the planes
// are periodic), as tile[r][tx][ty] -- ty contiguous as in memory, and a transform's plane on its own so that the 16
// lanes of an entry read 16 consecutive values.  (Four waves on one tile, not one: the tile's 16 KiB per workgroup
// bound a CU to ten single waves, too few to cover the staging loads -- 1.24 -> 1.00 ms per 32-channel C3 launch.)
// Then sixteen entries at a time, 16 lanes each: lane g < w owns the footprint's row
// y = i0y + g, walks the w columns with wx[k] handed round by shuffles, scales by wy[g]; a fixed
// butterfly combines the 16 lanes.  Every entry's Z goes once to the slot k_adj_accumulate reads: no atomics, and the
// result does not depend on the order of the entries inside a bin.
constexpr int T2_THREADS = 256;
template <typename T, int TP>
__global__ __launch_bounds__(T2_THREADS) void k_t2_gather(T1Args a, int P, int cnt, const unsigned char *__restrict__ recs,
                                                  const int *__restrict__ bin_start, const cplx<T> *__restrict__ grid,
                                                  cplx<T> *__restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char t2_smem[];
    cplx<T> *tile = reinterpret_cast<cplx<T> *>(t2_smem);
    const int bin = blockIdx.x;
    const int s = bin_start[bin], e1 = (int)min((int64_t)bin_start[bin + 1], a.ecap);
    if (s >= e1) return;  // (the whole workgroup)
    const int bx = bin % a.nb1, by = (bin / a.nb1) % a.nb1, f = bin / (a.nb1 * a.nb1);
    const int Tt = (1 << BINLOG) + a.w - 1, TT = Tt * Tt;
    const int x0 = (bx << BINLOG) - T1_PAD, y0 = (by << BINLOG) - T1_PAD;  // origins of the bin: [x0, x0 + 8)
    const int tid = threadIdx.x;
    for (int i = tid; i < TP * TT; i += T2_THREADS) {
        const int ty = i % Tt, tx = (i / Tt) % Tt, r = i / TT;
        int gx = x0 + tx, gy = y0 + ty;  // in [-PAD, n2 + 8 + w): one wrap either way
        gx += gx < 0 ? a.n2 : 0;
        gx -= gx >= a.n2 ? a.n2 : 0;
        gy += gy < 0 ? a.n2 : 0;
        gy -= gy >= a.n2 ? a.n2 : 0;
        tile[i] = grid[(((int64_t)f * TP + r) * a.n2 + out_pos(gx, P, cnt)) * a.n2 + gy];
    }
    __syncthreads();
    const int g = tid & 15, grp = tid >> 4;
    const int gc = min(g, a.w - 1);  // lanes beyond the kernel width carry zero weights
    for (int it = s; it < e1; it += T2_THREADS / 16) {
        const bool ok = it + grp < e1;
        const unsigned char *rec = recs + (int64_t)(ok ? it + grp : e1 - 1) * a.rec;
        const int4 h = *reinterpret_cast<const int4 *>(rec);
        const T *wr = reinterpret_cast<const T *>(rec + T1_HDR);
        const T wxg = g < a.w ? wr[g] : T(0), wyg = g < a.w ? wr[a.w + g] : T(0);
        const cplx<T> *t0 = tile + (h.x - x0) * Tt + (h.y - y0) + gc;
        cplx<T> acc[TP];
#pragma unroll
        for (int r = 0; r < TP; ++r) acc[r] = {T(0), T(0)};
        for (int k = 0; k < a.w; ++k) {
            const T wxk = __shfl(wxg, (tid & 48) + k, 64);  // (of this wave's lanes: the entry's group starts at lane tid & 48)
#pragma unroll
            for (int r = 0; r < TP; ++r) {
                const cplx<T> v = t0[r * TT + k * Tt];
                acc[r].re += wxk * v.re;
                acc[r].im += wxk * v.im;
            }
        }
#pragma unroll
        for (int r = 0; r < TP; ++r) {
            acc[r].re *= wyg;
            acc[r].im *= wyg;
            for (int off = 8; off > 0; off >>= 1) {
                acc[r].re += __shfl_xor(acc[r].re, off, 64);
                acc[r].im += __shfl_xor(acc[r].im, off, 64);
            }
        }
        if (ok && g == 0) {
            const int64_t p = h.z / a.nfg;  // ent = p nfg + f
#pragma unroll
            for (int r = 0; r < TP; ++r) z[((int64_t)f * TP + r) * a.cap + p] = acc[r];
        }
    }
}

// Brute-force type-3 sum on the device (independent checker; fp64 accumulation).
template <typename T>
__global__ void k_nudft_direct(int dim, int64_t M, const T *__restrict__ x, const T *__restrict__ y,
                               const T *__restrict__ z, const cplx<T> *__restrict__ c, int ntrans,
                               int64_t N, const T *__restrict__ s, const T *__restrict__ t,
                               const T *__restrict__ u, cplx<T> *__restrict__ out) {
    const int64_t k = blockIdx.x;
    const int tr = blockIdx.y;
    if (k >= N) return;
    const double sk = s[k], tk = dim > 1 ? (double)t[k] : 0.0, uk = dim > 2 ? (double)u[k] : 0.0;
    double ar = 0.0, ai = 0.0;
    for (int64_t j = threadIdx.x; j < M; j += blockDim.x) {
        double ph = sk * (double)x[j];
        if (dim > 1) ph += tk * (double)y[j];
        if (dim > 2) ph += uk * (double)z[j];
        double sn, cs;
        sincos(ph, &sn, &cs);
        const cplx<T> cv = c[(int64_t)tr * M + j];
        ar += (double)cv.re * cs - (double)cv.im * sn;
        ai += (double)cv.re * sn + (double)cv.im * cs;
    }
    __shared__ double rr[256], ri[256];
    rr[threadIdx.x] = ar;
    ri[threadIdx.x] = ai;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            rr[threadIdx.x] += rr[threadIdx.x + off];
            ri[threadIdx.x] += ri[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(int64_t)tr * N + k] = {(T)rr[0], (T)ri[0]};
}

// ---------------------------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------------------------
struct SimBase {
    virtual ~SimBase() = default;
    virtual void set_sources(int64_t nsrc, int nfreq, const void *eq, const void *flux, int pol_sky,
                             int on_device) = 0;
    virtual void set_times(int ntimes, const double *rot) = 0;
    virtual void set_topo(int ntimes, int64_t nsrc, const void *topo, int on_device) = 0;
    virtual void set_astrom(int ntimes, const double *astrom) = 0;
    virtual void set_freqs(int nfreq, const double *freqs) = 0;
    virtual void set_array(const double *R, int64_t nbls, const double *bls, int coplanar) = 0;
    virtual void set_array_type1(const double *basis, int64_t nbls, const int *bls_int, int n_modes) = 0;
    virtual void set_nbeams(int n) = 0;
    virtual void set_beam_airy(int b, double diameter, const double *jones_scale, double power_scale) = 0;
    virtual void set_reference_compat(int on) = 0;
    virtual void set_beam_table(int b, int nfreq_tab, int nza, int naz, double za_max,
                                const void *table, int order) = 0;
    virtual void set_beam_pairs(int npairs, const int *bi, const int *bj, const int64_t *off,
                                const int *idx, const signed char *flipped) = 0;
    virtual void set_basis(int nant, int K, int nfreq, const void *coefs, const int *ant1,
                           const int *ant2) = 0;
    virtual void set_chunking(int nchunks, double source_buffer) = 0;
    virtual void run(int t0, int t1, int f0, int f1, void *out, int out_on_device) = 0;
    // The row passes of a fit (residual_pass: fv_sim_run_residual, _gains, _jones; weight_pass: fv_sim_weight_block,
    // fv_sim_gain_weight_block, fv_sim_jones_weight_block): the calibration's kind and the caller's arrays, each a pointer
    // and whether it is a device pointer.  What a call does not take stays null.
    struct FitIn {
        const void *p = nullptr;
        int on_device = 0;
    };
    struct FitOut {
        void *p = nullptr;
        int on_device = 0;
    };
    struct FitArrays {
        FitIn data, weights, x, dx;  // x: the block's gains or matrices, dx: their direction
        FitOut gvis, grad;           // grad: the gradient (objective) or H block (product) with respect to x
    };
    virtual void residual_pass(Cal kind, int t0, int t1, int f0, int f1, const FitArrays &a, double *chi2_ft) = 0;
    virtual void weight_pass(Cal kind, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                             const FitArrays &a, double *q_ft) = 0;
    virtual void set_gain_pairs(int nant, const int *ant1, const int *ant2) = 0;
    virtual void run_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                             int gflux_on_device, int accumulate) = 0;
    virtual void run_basis_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                                   int gflux_on_device, void *gcoefs, int gcoefs_on_device, int accumulate) = 0;
    // basis: the entry point's kind of handle -- false fv_sim_run_position_adjoint / fv_sim_run_tangent (no basis beams),
    // true fv_sim_run_basis_position_adjoint / fv_sim_run_basis_position_tangent and fv_sim_run_basis_source_adjoint /
    // fv_sim_run_basis_source_tangent (a handle with fv_sim_set_basis)
    virtual void run_position_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gbls,
                                      int gbls_on_device, int accumulate, bool basis) = 0;
    virtual void run_source_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gtopo,
                                    int gtopo_on_device, int accumulate, bool basis) = 0;
    // fv_sim_run_sky_adjoint / fv_sim_run_basis_sky_adjoint: run_source_adjoint's pass with the flux gradient from its Z
    virtual void run_sky_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                                 int gflux_on_device, double *gtopo, int gtopo_on_device, int accumulate, bool basis) = 0;
    virtual void run_tangent(int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device, const double *dtopo,
                             int dtopo_on_device, void *out, int out_on_device, bool basis) = 0;
    virtual void run_basis_tangent(int t0, int t1, int f0, int f1, const void *dcoefs, int dcoefs_on_device, int ndir, void *out,
                                   int out_on_device) = 0;
    // Host destination of the next run (fv_sim_run_into): `out` is then a block INSIDE a larger array -- channel f of
    // the block starts f * out_f_stride elements after `out` (0: the block is contiguous) -- and with out_shared other
    // processes write the rest of that array (a sharded run's ranks filling one shared result): the pinning helper must
    // then neither write to it nor register more than the block's own runs.  Reset by every run.
    int64_t out_f_stride = 0;
    int out_shared = 0;
    // fv_sim_set_adjoint_path (0: the swapped type-3 transform, 1: the type-2 transform of a lattice handle) and what the
    // last run_adjoint took (fv_sim_last_adjoint_path: 0 none yet, 2, 3)
    int adjoint_path = 0;
    int last_adjoint_path = 0;
    virtual void sync() = 0;
    virtual void stats(double *v, int n) = 0;
    virtual void reset_stats() = 0;
    virtual void enable_timing(int on) = 0;
    virtual void timing(double *ms, int n) = 0;
};

enum { TM_SPREAD = 0, TM_FFT, TM_INTERP, TM_STRENGTHS, TM_PREP, TM_COUNT };
// slots of fv_sim_stats, in the order include/fftvis_hip.h documents them
enum {
    ST_SPREAD_LAUNCHES = 0, ST_SPREAD_CELLS, ST_SOURCE_VISITS, ST_FFT_CELLS, ST_GATHERED, ST_ABOVE_HORIZON, ST_N2X, ST_N2Y,
    ST_NA_XY, ST_W, ST_SIGMA, ST_MAX_ABOVE_HORIZON, ST_FFT_FLOPS, ST_N2_3, ST_NA_3, ST_HEIGHT_TERMS, ST_LANES, ST_LANE_MODE,
    ST_LIGHT_FROM, ST_LIGHTER_FROM
};

template <typename T>
class Sim : public SimBase {
    int device;
    hipStream_t stream = nullptr;
    double eps, sigma;       // sigma: the caller's upsampling factor, 0 = chosen per run (see run())
    double sigma_run = 2.0;  // the factor the last run used
    bool polarized;
    int tpol;

    int64_t nsrc = 0;
    int nfreq_cat = 0;
    bool pol_sky = false;
    DevBuf d_eq, d_flux;

    std::vector<Rot9> rots;
    int ntimes_topo = 0;  // > 0: per-time topocentric unit vectors were supplied instead
    std::vector<Astrom> astroms;  // non-empty: per-time astrometry contexts, applied on the device (k_astrom_topo)
    DevBuf d_topo;        // (ntimes, 3, nsrc) T
    std::vector<double> freqs;
    DevBuf d_freqs;

    Rot9 rplane{};
    int64_t nbls = 0;
    bool coplanar = true;
    std::vector<double> h_bls;  // (3, nbls) seconds
    bool order_pairs = true;    // set_beam_pairs visits a pair's baselines in (u, v) order
    DevBuf d_bls;               // (3, nbls) T

    int beam_order = 1;  // interpolation order of the tabulated beams (1 or 3)
    struct Beam {
        int kind = -1;
        double diameter = 0;
        double js[8] = {1, 0, 1, 0, 1, 0, 1, 0}, ps = 1;  // Airy: Jones-slot factors, power factor
        int nfreq_tab = 0, nza = 0, naz = 0;
        double za_max = 0;
        std::unique_ptr<DevBuf> table;
        bool real_valued = true;  // every Jones entry has zero imaginary part (Airy; tables are scanned at upload)
    };
    std::vector<Beam> beams;

    struct Pair {
        int bi, bj;
        int64_t n;
        bool trivial;  // all baselines in order, nothing flipped
        std::unique_ptr<DevBuf> idx, flip;
        // the list in the CALLER's order (usually increasing baseline index): what the lattice path's mode pick walks --
        // its reads are a few thousand distinct modes of a plane that sits in L2 whatever the order, its WRITES are 16 bytes
        // per (baseline, product) and want neighbouring threads on neighbouring baselines
        bool trivial0 = false;
        std::unique_ptr<DevBuf> idx0, flip0;
        // Redundant baselines: runs of the (u, v)-ordered list whose sign-adjusted vectors agree (build_unique) are ONE
        // target of the gather.  h_idx / h_flip: the list as visited (host copy); ustart: nu + 1 run starts (device).
        std::vector<int> h_idx, h_ustart, h_upairs;  // (h_upairs: host copy of upairs, for the direct y sums' point map)
        std::vector<signed char> h_flip;
        bool sorted = false;  // the list is visited in (u, v) order
        std::unique_ptr<DevBuf> ustart, upairs;  // run starts; (packed runs) pairs of runs b / -b that share one gather item
        int64_t nu = 0, nitems = 0;               // runs; gather items (= runs unless paired)
        double utol = -1.0;
        int udims = 3;  // components compared when runs were built (2 under height terms: b_z is per member there)
        int upairs_herm = -1;
        double btc[3], B[3];   // tight box of its (sign-adjusted) baselines: centre, half-width [s]
        double Bs[3];          // half-width of the box made symmetric about 0
        int herm = 0;          // this run packs its strengths into two transforms: 1 Hermitian, 2 all real (per run)
        bool mirror = false;   // this run also gathers at the mirror targets -b (exact eigenbeam (l, k) terms)
        const double *box_c() const { return herm || mirror ? zero3 : btc; }
        const double *box_B() const { return herm || mirror ? Bs : B; }
        // the adjoint's NUFFT sources: the first member's sign-adjusted vector of every run, (dim, nu) T, built for
        // target-data version adj_serial
        std::unique_ptr<DevBuf> adj_pos;
        int64_t adj_serial = -1;
        int64_t adj_np = 0;  // sources in adj_pos: nu, or 2 nu with the mirrored set of the exact basis form
        // the type-2 adjoint's mode -> run table (mode_cells): na^2 + 1 cell starts, then the runs cell by cell
        std::unique_ptr<DevBuf> t2_cells;
        int64_t t2_serial = -1;
        int t2_na = 0;
    };
    static constexpr double zero3[3] = {0.0, 0.0, 0.0};
    std::vector<Pair> pairs;
    // Source-axis chunking (reference cpu_simulate.py:939: `for chunk in range(nchunks)` inside the time
    // loop, visibilities accumulate with +=): per-time scratch is sized by one chunk, the catalog stays
    // resident.  source_buffer = fraction of a chunk the above-horizon arrays can hold (matvis sizes its
    // buffers the same way and raises when a chunk has more sources above the horizon).
    int src_chunks = 1;
    double source_buffer = 1.0;
    int nbasis = 0;  // > 0: eigenbeam mode
    // type-1 (lattice) mode
    bool type1 = false;
    int t1_nmodes = 0;
    DevBuf d_blint;  // (2, nbls) int
    DevBuf t1_meta[2], t1_binstart[2], t1_rec[2], t1_cs, t1_dec;  // [2]: pipelined (time, batch) units
    std::unique_ptr<Nufft3<T>> t1fft;
    DevBuf d_coefs, d_ant1, d_ant2;

    // Per-time scratch lives in a lane.  Small problems run consecutive time steps on two lanes
    // (two streams) so that one step's launch ramps and tails overlap the other's kernels.
    static constexpr int NCLS = 3;  // plan classes of a lane
    struct Lane {
        hipStream_t stream = nullptr;
        bool own_stream = false;
        hipEvent_t done = nullptr;
        hipEvent_t prep_done = nullptr, heavy_done = nullptr;  // pipelined mode (see run())
        bool heavy_pending = false;
        // the type-3 plans by class: 0 the run's own, 1 and 2 the LIGHT height terms' (see light_classes): looser
        // tolerances, sigma = 1.25; with the (time, chunk) and geometry their sources were last binned for
        std::unique_ptr<Nufft3<T>> plan[NCLS];
        int binned_ti[NCLS] = {-1, -1, -1};
        int64_t binned_serial[NCLS] = {-1, -1, -1};
        DevBuf d_xyz, d_az, d_za, d_srcidx, d_blockcnt, d_blockoff, d_scan_tot, d_scan_off, d_enu;
        // adjoint (run_adjoint): the transform with the roles swapped, its strengths, its values at the directions and
        // this lane's fp64 gradient accumulator
        std::unique_ptr<Nufft3<T>> adj;
        DevBuf d_adj_q, d_adj_z, d_adj_acc;
        DevBuf d_gs;  // basis adjoint, coefficient pass: this lane's inner products S (k_interp<.., GRAD>)
        // type-2 adjoint (lattice handles): the pruned FFT the other way round, its deconvolution table over the input
        // modes, and this lane's entry-sort buffers (t1_sort)
        std::unique_ptr<Nufft3<T>> adj2;
        DevBuf d_t2_dec, d_t2_meta, d_t2_binstart, d_t2_rec;
    };
    Lane lanes[4];  // [2], [3]: second pair of the gang mode (see run())
    int lane_mode = -1;       // 0 one stream per lane, 1 pipelined, 2 pipelined gangs: what the lanes last ran as
    int64_t lane_serial = 0;  // units processed in that mode (lane rotation continues across runs)
    hipStream_t prep_stream = nullptr;  // low priority: per-time preparation of the next step
    // Host output of a large run (drain_*): the caller's array is pinned in place while the GPU computes, and every
    // finished time step leaves through this stream beside the later steps' kernels.
    hipStream_t copy_stream = nullptr;
    std::vector<hipEvent_t> drain_events;  // "time step(s) finished", reused from run to run
    struct DrainItem {
        hipEvent_t ev;
        int t, n;  // time steps [t, t + n) of the run's block
    };
    hipEvent_t ev_start = nullptr;
    DevBuf d_out, d_mhist;
    DevBuf d_adj_g, d_adj_gf;  // adjoint: host G block / host gradient staged on the device
    DevBuf d_adj_gc;           // basis adjoint: host coefficient gradient staged on the device
    DevBuf d_tan_w, d_tan_dt;  // tangent: the rounds' weights (RunPlan::tan_w), host dtopo staged on the device
    DevBuf d_res_d, d_res_w;   // fused objective: host data / host weights staged on the device
    DevBuf d_res_sum;          // fused objective: the blocks' partial sums, the rows' sums and the two bad-input counters
    DevBuf d_res_g, d_res_gg;  // gains: a block's host gains staged on the device / the gain gradient of a host destination
    DevBuf d_res_dg;           // gains: a block's host gain direction staged on the device (fv_sim_gain_weight_block)
    DevBuf d_res_terms;        // Jones gains: the rows' fp64 terms of a block (fv_sim_run_residual_jones)
    GainPairs gain_pairs;      // gains: the antenna pair of every baseline and the incidence lists (fv_sim_set_gain_pairs)
    DevBuf d_bt_d, d_bt_out;   // basis tangent: host directions D / the (ndir, ...) output of a host destination, on the device
    DevBuf d_csr_start, d_csr;  // basis mode: per antenna, its baselines as 2 b + role (k_coef_reduce)
    int nant_basis = 0;
    // sticky device-side error counters, read at every host synchronisation point (check_errors):
    // [0] sources outside the planned box or with NaN coordinates (k_bin_count), [1] type-1 entries
    // dropped because the entry buffers overflowed (k_t1_bin), [2] above-horizon sources that did not
    // fit source_buffer x chunk size (k_horizon_compact), [3] footprint columns missing from a column plan (k_interp),
    // [4] NaN entries of the adjoint's visibility-shaped input (k_adj_strengths)
    DevBuf d_err;
    static constexpr int NERR = 5;
    std::vector<std::pair<int, double>> mhist_log;  // (time index, transforms spread) per processed time

    // stats / timing
    double st[24] = {0};
    int timing_level = 0;  // 1: spread only, sampled (events ride on the dispatches); 3: the same on every spread launch; 2: every kernel family
    int64_t targets_serial = 1;  // version of the device-side target data (baselines, frequencies, pair lists)
    struct Ev {
        hipEvent_t a, b;
        int kind;
    };
    std::vector<Ev> ev_pool;
    size_t ev_used = 0;
    double tm[TM_COUNT] = {0};
    // level 1 attaches events to the spread launches of one time step in TIMING_STRIDE (16; the 9th of
    // each 16, a steady-state one rather than the first after the run's set-up) only (all
    // frequency groups of that step, so the sample is representative): even dispatch-attached
    // events leave ~5-8 us of idle queue on either side of a launch
    static constexpr int TIMING_STRIDE = 16;
    double spread_timed = 0;

    int dim() const { return coplanar ? 2 : 3; }

    size_t ev_slot(int kind) {
        if (ev_used == ev_pool.size()) {
            Ev e;
            FV_HIP(hipEventCreate(&e.a));
            FV_HIP(hipEventCreate(&e.b));
            e.kind = kind;
            ev_pool.push_back(e);
        }
        ev_pool[ev_used].kind = kind;
        return ev_used++;
    }
    size_t ev_begin(int kind, hipStream_t st_) {
        if (timing_level != 2) return (size_t)-1;
        const size_t i = ev_slot(kind);
        FV_HIP(hipEventRecord(ev_pool[i].a, st_));
        return i;
    }
    void ev_end(size_t i, hipStream_t st_) {
        if (i == (size_t)-1) return;
        FV_HIP(hipEventRecord(ev_pool[i].b, st_));
    }
    void ev_collect() {
        for (size_t i = 0; i < ev_used; ++i) {
            float ms = 0;
            FV_HIP(hipEventElapsedTime(&ms, ev_pool[i].a, ev_pool[i].b));
            tm[ev_pool[i].kind] += ms;
        }
        ev_used = 0;
    }

   public:
    Sim(int device_, double eps_, double sigma_, int polarized_)
        : device(device_), eps(eps_), sigma(sigma_), polarized(polarized_ != 0),
          tpol(polarized_ ? 4 : 1) {
        FV_HIP(hipSetDevice(device));
        int prio_least = 0, prio_greatest = 0;
        FV_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        FV_HIP(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio_greatest));
        lanes[0].stream = stream;
        // the second lane's stream has the main stream's priority: two free-running lanes then share the dispatcher like two
        // processes do (with a lower priority the second lane only ever filled the first one's tails)
        FV_HIP(hipStreamCreateWithPriority(&lanes[1].stream, hipStreamNonBlocking,
                                           std::getenv("FFTVIS_HIP_LANE1_LOW") ? (prio_least + prio_greatest) / 2 : prio_greatest));
        lanes[1].own_stream = true;
        // (streams of a third and fourth free-running lane are made on demand, run(): streams share the few hardware
        // queues, and two more of them at creation put the main stream and the low-priority preparation stream of the
        // pipelined small-grid mode on one queue -- C2 1.43 -> 3.6 ms per step)
        FV_HIP(hipStreamCreateWithPriority(&prep_stream, hipStreamNonBlocking, prio_least));
        for (Lane &L : lanes) FV_HIP(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        for (Lane &L : lanes) {
            FV_HIP(hipEventCreateWithFlags(&L.prep_done, hipEventDisableTiming));
            FV_HIP(hipEventCreateWithFlags(&L.heavy_done, hipEventDisableTiming));
        }
        FV_HIP(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
        d_err.reserve(NERR * sizeof(int));
        FV_HIP(hipMemsetAsync(d_err.p, 0, NERR * sizeof(int), stream));
        for (int i = 0; i < 9; ++i) rplane.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    ~Sim() override {
        (void)hipSetDevice(device);
        for (Lane &L : lanes) {
            for (auto &P : L.plan) P.reset();
            L.adj.reset();
            L.adj2.reset();
            if (L.done) (void)hipEventDestroy(L.done);
            if (L.prep_done) (void)hipEventDestroy(L.prep_done);
            if (L.heavy_done) (void)hipEventDestroy(L.heavy_done);
            if (L.own_stream && L.stream) (void)hipStreamDestroy(L.stream);
        }
        if (prep_stream) (void)hipStreamDestroy(prep_stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (hipEvent_t e : drain_events) (void)hipEventDestroy(e);
        if (ev_start) (void)hipEventDestroy(ev_start);
        for (auto &e : ev_pool) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }

    void upload(DevBuf &dst, const void *src, size_t bytes, int on_device) {
        dst.reserve(std::max<size_t>(bytes, 16));
        if (bytes)
            FV_HIP(hipMemcpyAsync(dst.p, src, bytes,
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        FV_HIP(hipStreamSynchronize(stream));
    }

    void set_sources(int64_t n, int nfreq, const void *eq, const void *flux, int ps,
                     int on_device) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(n >= 0 && nfreq >= 1, "bad catalog shape");
        FV_REQUIRE(n < (int64_t)1 << 31, "catalog too large for 32-bit source indices");
        FV_REQUIRE(!ps || polarized, "polarized sky needs a polarized engine (cpu/utils.py:56-66)");
        nsrc = n;
        nfreq_cat = nfreq;
        pol_sky = ps != 0;
        upload(d_eq, eq, sizeof(T) * 3 * n, on_device);
        upload(d_flux, flux, (pol_sky ? sizeof(T) * 8 : sizeof(T)) * (size_t)n * nfreq, on_device);
    }
    void set_astrom(int ntimes, const double *astrom) override {
        mhist_log.clear();
        ntimes_topo = 0;
        rots.assign(ntimes, Rot9{{1, 0, 0, 0, 1, 0, 0, 0, 1}});  // the horizon kernels then read finished ENU vectors
        astroms.resize(ntimes);
        std::memcpy(astroms.data(), astrom, sizeof(Astrom) * (size_t)ntimes);
        for (const Astrom &a : astroms) {
            FV_REQUIRE(a.em > 0 && a.bm1 > 0, "astrometry context: em (Sun distance, au) and bm1 must be positive");
            for (int i = 0; i < 31; ++i) FV_REQUIRE(std::isfinite(reinterpret_cast<const double *>(&a)[i]), "astrometry context: not finite");
        }
    }
    void set_times(int ntimes, const double *rot) override {
        mhist_log.clear();  // entries index the previous configuration's time axis
        ntimes_topo = 0;
        astroms.clear();
        rots.resize(ntimes);
        for (int i = 0; i < ntimes; ++i) std::memcpy(rots[i].m, rot + 9 * i, 9 * sizeof(double));
    }
    void set_topo(int ntimes, int64_t n, const void *topo, int on_device) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(n == nsrc, "topo source count != catalog (set_sources first)");
        mhist_log.clear();
        ntimes_topo = ntimes;
        astroms.clear();
        rots.assign(ntimes, Rot9{{1, 0, 0, 0, 1, 0, 0, 0, 1}});
        upload(d_topo, topo, sizeof(T) * 3 * (size_t)n * ntimes, on_device);
    }
    // (Re-setting what the handle already holds -- a caller that simulates the same array again and again -- leaves the
    // version of the target data alone: the column plans, unique-target runs and fused-gather records stay valid.)
    void set_freqs(int nf, const double *f) override {
        if ((size_t)nf == freqs.size() && nf > 0 && std::memcmp(freqs.data(), f, sizeof(double) * nf) == 0) return;
        ++targets_serial;  // tabulated target records (fused gather) are stale now
        FV_HIP(hipSetDevice(device));
        freqs.assign(f, f + nf);
        upload(d_freqs, f, sizeof(double) * nf, 0);
    }
    void set_array(const double *R, int64_t nb, const double *bls, int cop) override {
        if (!type1 && nbasis == 0 && nb == nbls && nb > 0 && coplanar == (cop != 0) && h_bls.size() == (size_t)3 * nb &&
            std::memcmp(rplane.m, R, 9 * sizeof(double)) == 0 && std::memcmp(h_bls.data(), bls, sizeof(double) * 3 * nb) == 0)
            return;  // the same array: the pair lists (and everything planned from them) stay
        ++targets_serial;  // tabulated target records (fused gather) are stale now
        FV_HIP(hipSetDevice(device));
        std::memcpy(rplane.m, R, 9 * sizeof(double));
        nbls = nb;
        nbasis = 0;
        type1 = false;
        coplanar = cop != 0;
        h_bls.assign(bls, bls + 3 * nb);
        std::vector<T> tmp(3 * nb);
        for (int64_t i = 0; i < 3 * nb; ++i) tmp[i] = (T)bls[i];
        upload(d_bls, tmp.data(), sizeof(T) * 3 * nb, 0);
        pairs.clear();
        gain_pairs.nbls = -1;  // (the pairs belonged to the previous baselines)
    }
    // Lattice array (cpu_simulate.py:661-681): integer baselines, n_modes = 2 max|bl| + 1 and the
    // basis matrix in seconds; topo is rotated by basis^T instead of the plane rotation (:964-965).
    void set_array_type1(const double *basis, int64_t nb, const int *bls_int, int n_modes) override {
        ++targets_serial;  // tabulated target records (fused gather) are stale now
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(n_modes >= 1 && n_modes % 2 == 1, "n_modes must be odd");
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rplane.m[3 * i + j] = basis[3 * j + i];  // basis^T
        nbls = nb;
        nbasis = 0;
        coplanar = true;
        type1 = true;
        t1_nmodes = n_modes;
        gain_pairs.nbls = -1;  // (the pairs belonged to the previous baselines)
        h_bls.assign(3 * nb, 0.0);
        for (int64_t k = 0; k < nb; ++k) {
            FV_REQUIRE(std::abs(bls_int[k]) <= n_modes / 2 && std::abs(bls_int[nb + k]) <= n_modes / 2,
                       "integer baseline outside the mode range");
            h_bls[k] = bls_int[k];
            h_bls[nb + k] = bls_int[nb + k];
        }
        upload(d_blint, bls_int, sizeof(int) * 2 * nb, 0);
        pairs.clear();
    }
    // SURVEY App. B Q1 / Q2.  on (default): the reference's forms -- flipped baselines of a two-beam pair are
    // conjugated but their 2 x 2 block is not transposed (cpu_simulate.py:298); the eigenbeam (l, k) term reuses
    // V_kl(b)^T (:464-468, exact for real basis beams only).  off: V_ji(b) = V_ij(-b)^H and
    // V_lk(b) = conj(V_kl(-b))^T -- the transform is evaluated at -b as well.
    bool reference_compat = true;
    void set_reference_compat(int on) override { reference_compat = on != 0; }
    void set_nbeams(int n) override {
        beams.clear();
        beams.resize(n);
    }
    void set_beam_airy(int b, double diameter, const double *jones_scale, double power_scale) override {
        FV_REQUIRE(b >= 0 && b < (int)beams.size(), "beam index out of range");
        Beam &bm = beams[b];
        bm.kind = 0;
        bm.diameter = diameter;
        bm.ps = power_scale;
        bm.real_valued = true;
        for (int i = 0; i < 8; ++i) {
            bm.js[i] = jones_scale ? jones_scale[i] : (i % 2 ? 0.0 : 1.0);
            FV_REQUIRE(bm.js[i] == bm.js[i], "NaN in the Airy Jones factors");
            if (i % 2 && bm.js[i] != 0.0) bm.real_valued = false;
        }
    }
    void set_beam_table(int b, int nft, int nza, int naz, double za_max, const void *table,
                        int order) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(b >= 0 && b < (int)beams.size(), "beam index out of range");
        FV_REQUIRE(nza >= 2 && naz >= 1 && nft >= 1 && za_max > 0, "bad beam table shape");
        FV_REQUIRE(order >= 0 && order <= 5, "beam interpolation order must be 0 .. 5");
        for (size_t i = 0; i < beams.size(); ++i)  // one spline_opts per simulation (cpu_simulate.py:557)
            FV_REQUIRE((int)i == b || beams[i].kind != 1 || beam_order == order,
                       "all tabulated beams of a handle share one interpolation order");
        beam_order = order;
        Beam &bm = beams[b];
        bm.kind = 1;
        bm.real_valued = true;
        if (polarized) {  // Jones tables with no imaginary part anywhere make every coherency product real
            const double *tv = static_cast<const double *>(table);
            const size_t nc = (size_t)nft * 4 * nza * naz;
            for (size_t i = 0; i < nc && bm.real_valued; ++i) bm.real_valued = tv[2 * i + 1] == 0.0;
        }
        bm.nfreq_tab = nft;
        bm.nza = nza;
        bm.naz = naz;
        bm.za_max = za_max;
        bm.table.reset(new DevBuf());
        const size_t per = polarized ? 4 * 16 : 8;  // complex128 Jones or float64 power
        if (!polarized) {
            upload(*bm.table, table, per * (size_t)nft * nza * naz, 0);
        } else {  // Jones tables live interleaved on the device (see eval_jones)
            DevBuf tmp;
            upload(tmp, table, per * (size_t)nft * nza * naz, 0);
            bm.table->reserve(per * (size_t)nft * nza * naz);
            const int64_t nodes = (int64_t)nza * naz;
            hipLaunchKernelGGL(k_jones_interleave, dim3((unsigned)cdiv(nodes * nft, 256)), dim3(256), 0, stream,
                               tmp.as<cplx<double>>(), bm.table->template as<cplx<double>>(), nodes, (int64_t)nft);
            FV_HIP(hipStreamSynchronize(stream));  // tmp goes out of scope
        }
        bspline_prefilter(bm.table->template as<double>(), nft, nza, naz, polarized ? 8 : 1, order, stream);
    }
    std::vector<int> in_bi, in_bj, in_idx;  // the caller's last pair lists, as given
    std::vector<int64_t> in_off;
    std::vector<signed char> in_fl;
    bool in_ordered = true;
    void set_beam_pairs(int np, const int *bi, const int *bj, const int64_t *off, const int *idx,
                        const signed char *flipped) override {
        {
            const int64_t tot = np > 0 ? off[np] : 0;
            if (!pairs.empty() && (int)pairs.size() == np && in_ordered == order_pairs && (int)in_bi.size() == np &&
                (int64_t)in_idx.size() == tot && std::equal(bi, bi + np, in_bi.begin()) && std::equal(bj, bj + np, in_bj.begin()) &&
                std::equal(off, off + np + 1, in_off.begin()) && std::equal(idx, idx + tot, in_idx.begin()) &&
                std::equal(flipped, flipped + tot, in_fl.begin()))
                return;  // the same lists on the same array (set_array clears the pairs when the array changes)
            in_bi.assign(bi, bi + np);
            in_bj.assign(bj, bj + np);
            in_off.assign(off, off + np + 1);
            in_idx.assign(idx, idx + tot);
            in_fl.assign(flipped, flipped + tot);
            in_ordered = order_pairs;
        }
        ++targets_serial;
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nbls > 0 || np == 0, "set_array first");
        pairs.clear();
        for (int p = 0; p < np; ++p) {
            Pair pr;
            pr.bi = bi[p];
            pr.bj = bj[p];
            pr.n = off[p + 1] - off[p];
            const int *ix = idx + off[p];
            const signed char *fl = flipped + off[p];
            for (int64_t k = 0; k < pr.n; ++k) FV_REQUIRE(ix[k] >= 0 && ix[k] < nbls, "baseline index out of range");
            // The list is visited in order of the (flipped) baseline vector: redundant baselines -- most of a regular
            // array's -- then sit next to each other, the gather hands neighbouring items to one XCD, and they read
            // their common grid lines through one L2 (C3: 0.31 -> 0.25 ms per launch).  The order of a list is free:
            // every baseline writes its own output slot.
            static const bool keep_order = std::getenv("FFTVIS_HIP_NO_TARGET_SORT") != nullptr;
            pr.trivial0 = pr.n == nbls;
            for (int64_t k = 0; k < pr.n && pr.trivial0; ++k) pr.trivial0 = ix[k] == k && !fl[k];
            if (!pr.trivial0 && pr.n && type1) {
                pr.idx0.reset(new DevBuf());
                pr.flip0.reset(new DevBuf());
                upload(*pr.idx0, ix, sizeof(int) * pr.n, 0);
                upload(*pr.flip0, fl, pr.n, 0);
            }
            std::vector<int> six(ix, ix + pr.n);
            std::vector<signed char> sfl(fl, fl + pr.n);
            if (!keep_order && order_pairs && pr.n > 1) {
                double bmax = 0;
                for (int64_t k = 0; k < pr.n; ++k)
                    bmax = std::max({bmax, std::fabs(h_bls[ix[k]]), std::fabs(h_bls[(size_t)nbls + ix[k]])});
                const double q = 1e-7 * std::max(bmax, 1e-300);  // ties for vectors equal up to rounding
                std::vector<std::pair<int64_t, int64_t>> key(pr.n);
                std::vector<int64_t> ord(pr.n);
                for (int64_t k = 0; k < pr.n; ++k) {
                    const double sg = fl[k] ? -1.0 : 1.0;
                    key[k] = {(int64_t)std::llround(sg * h_bls[ix[k]] / q), (int64_t)std::llround(sg * h_bls[(size_t)nbls + ix[k]] / q)};
                    ord[k] = k;
                }
                std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
                for (int64_t k = 0; k < pr.n; ++k) {
                    six[k] = ix[ord[k]];
                    sfl[k] = fl[ord[k]];
                }
            }
            ix = six.data();
            fl = sfl.data();
            pr.trivial = pr.n == nbls;
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            for (int64_t k = 0; k < pr.n; ++k) {
                if (ix[k] != k || fl[k]) pr.trivial = false;
                const double sg = fl[k] ? -1.0 : 1.0;
                for (int d = 0; d < 3; ++d) {
                    const double v = sg * h_bls[(size_t)d * nbls + ix[k]];
                    lo[d] = std::min(lo[d], v);
                    hi[d] = std::max(hi[d], v);
                }
            }
            for (int d = 0; d < 3; ++d) {
                pr.btc[d] = pr.n ? 0.5 * (lo[d] + hi[d]) : 0.0;
                pr.B[d] = pr.n ? 0.5 * (hi[d] - lo[d]) * (1.0 + 1e-12) : 0.0;
                pr.Bs[d] = pr.n ? std::max(std::fabs(lo[d]), std::fabs(hi[d])) * (1.0 + 1e-12) : 0.0;
            }
            if (!pr.trivial && pr.n) {
                pr.idx.reset(new DevBuf());
                pr.flip.reset(new DevBuf());
                upload(*pr.idx, ix, sizeof(int) * pr.n, 0);
                upload(*pr.flip, fl, pr.n, 0);
            }
            pr.sorted = !keep_order && order_pairs && pr.n > 1;
            pr.h_idx = std::move(six);
            pr.h_flip = std::move(sfl);
            pairs.push_back(std::move(pr));
        }
    }

    // Redundant baselines are one target.  A regular array repeats most of its baseline vectors (HERA-350: 61 075
    // baselines, 7 957 distinct vectors), the visibility of a (beam pair, baseline vector) does not depend on WHICH
    // antennas form it, and the list is already visited in (u, v) order: runs of entries whose sign-adjusted vectors
    // agree to `tol` seconds in every component -- tol = what moves the phase 2 pi nu b . x by at most 1e-3 eps at the
    // run's highest frequency, i.e. far below the transform's own error; exact duplicates always qualify -- are gathered
    // once (k_interp walks the run for the output slots).  Compared with the run's FIRST entry, so runs cannot drift.
    // FFTVIS_HIP_NO_TARGET_DEDUP=1 turns it off.  nd: components compared (2 under height terms: a run shares (u, v)
    // only, every member brings its own b_z).
    void build_unique(Pair &p, double tol, int nd) {
        const bool off = std::getenv("FFTVIS_HIP_NO_TARGET_DEDUP") != nullptr;  // read per run: tests flip it
        if (off) tol = -2.0;
        if (p.utol == tol && p.udims == nd) return;
        p.utol = tol;
        p.udims = nd;
        p.ustart.reset();
        p.upairs.reset();
        p.upairs_herm = -1;  // (pair_mirror_runs starts over on the new runs)
        p.h_upairs.clear();
        p.h_ustart.clear();
        p.nu = p.nitems = p.n;
        ++targets_serial;  // column plans were built from the old runs
        if (off || !p.sorted) return;
        std::vector<int> st(1, 0);
        auto comp = [&](int64_t k, int d) { return (p.h_flip[k] ? -1.0 : 1.0) * h_bls[(size_t)d * nbls + p.h_idx[k]]; };
        for (int64_t k = 1; k < p.n; ++k) {
            const int64_t k0 = st.back();
            bool same = true;
            for (int d = 0; d < nd && same; ++d) same = std::fabs(comp(k, d) - comp(k0, d)) <= tol;
            if (!same) st.push_back((int)k);
        }
        st.push_back((int)p.n);
        const int64_t nu = (int64_t)st.size() - 1;
        if (nu * 10 > p.n * 9) return;  // (almost) nothing repeats: the plain list
        p.ustart.reset(new DevBuf());
        upload(*p.ustart, st.data(), sizeof(int) * st.size(), 0);
        p.nu = nu;
        p.h_ustart = std::move(st);
    }

    // Packed runs gather every target at s and at -s: the run of baselines b and the run of baselines -b want the same
    // two evaluations and share one item (k_interp: upairs).  Runs are matched through a hash of their vectors rounded
    // to 4 tol (the 27 neighbouring cells are searched: either vector may sit next to a rounding boundary).
    void pair_mirror_runs(Pair &p, double tol) {
        const bool want = p.herm != 0 && p.ustart && tol > 0.0 && !std::getenv("FFTVIS_HIP_NO_TARGET_PAIRS");
        const int nd = p.udims;
        if (p.upairs_herm == (want ? nd : 0)) return;
        p.upairs_herm = want ? nd : 0;
        p.upairs.reset();
        p.h_upairs.clear();
        p.nitems = p.nu;
        ++targets_serial;
        if (!want) return;
        const double q = 4.0 * tol;
        struct Key {
            int64_t a, b, c;
            bool operator==(const Key &o) const { return a == o.a && b == o.b && c == o.c; }
        };
        struct Hash {
            size_t operator()(const Key &k) const { return (size_t)(k.a * 0x9E3779B97F4A7C15ull) ^ (size_t)(k.b * 0xC2B2AE3D27D4EB4Full) ^ (size_t)(k.c * 0x165667B19E3779F9ull); }
        };
        auto vec = [&](int64_t u, int d) {
            const int64_t kl = p.h_ustart[u];
            return (p.h_flip[kl] ? -1.0 : 1.0) * h_bls[(size_t)d * nbls + p.h_idx[kl]];
        };
        std::unordered_map<Key, int, Hash> at;
        at.reserve((size_t)p.nu * 2);
        auto cell2 = [&](double v) { return nd > 2 ? (int64_t)std::llround(v / q) : (int64_t)0; };
        for (int64_t u = 0; u < p.nu; ++u) at[Key{(int64_t)std::llround(vec(u, 0) / q), (int64_t)std::llround(vec(u, 1) / q), cell2(vec(u, 2))}] = (int)u;
        std::vector<int> partner((size_t)p.nu, -1), items;
        for (int64_t u = 0; u < p.nu; ++u) {
            if (partner[u] >= 0) continue;
            const int64_t k0 = std::llround(-vec(u, 0) / q), k1 = std::llround(-vec(u, 1) / q), k2 = cell2(-vec(u, 2));
            int best = -1;
            for (int da = -1; da <= 1 && best < 0; ++da)
                for (int db = -1; db <= 1 && best < 0; ++db)
                    for (int dc = (nd > 2 ? -1 : 0); dc <= (nd > 2 ? 1 : 0) && best < 0; ++dc) {
                        auto it = at.find(Key{k0 + da, k1 + db, k2 + dc});
                        if (it == at.end()) continue;
                        const int v = it->second;
                        if (v == (int)u || partner[v] >= 0) continue;
                        bool same = true;
                        for (int d = 0; d < nd && same; ++d) same = std::fabs(vec(v, d) + vec(u, d)) <= tol;
                        if (same) best = v;
                    }
            if (best >= 0) {
                partner[u] = best;
                partner[best] = (int)u;
            }
        }
        for (int64_t u = 0; u < p.nu; ++u) {
            if (partner[u] >= 0 && partner[u] < (int)u) continue;  // listed with its partner
            items.push_back((int)u);
            items.push_back(partner[u]);
        }
        if ((int64_t)items.size() / 2 == p.nu) return;  // no mirror pairs
        p.upairs.reset(new DevBuf());
        upload(*p.upairs, items.data(), sizeof(int) * items.size(), 0);
        p.nitems = (int64_t)items.size() / 2;
        p.h_upairs = std::move(items);
    }

    // Column plan (Nufft3::arm_columns): which columns of the transform's first dimension the targets of one (frequency
    // group, beam pair) read at all, per frequency -- the footprints of the distinct target vectors (and of their
    // mirror images where the run gathers at -s too), exactly as k_interp places them; a footprint whose first column
    // is within 1e-6 of a rounding boundary takes both candidates.  Compact numbers follow the residue-major
    // position order, so that a residue job of the x-pass stores runs of neighbouring compact columns.  Host
    // arithmetic, once per (targets, group geometry); kept for later runs.  Not used when it would keep more than
    // 85 % of the columns (arrays without repeated baseline vectors).  FFTVIS_HIP_NO_COLUMN_PLAN=1 turns it off.
    struct ColPlan {
        int64_t serial;
        int pair, fa, fb, nos, sP, cnt, n2, no, w;
        double h, btc;
        bool both;
        DevBuf tab, xtab;  // the gather's table (1 + compact column) and the x-pass's (1 + element index of that column)
        std::vector<int> h_tab;  // host copy of tab (Sim::ydirect_plan locates its columns through it)
        int yna = 0, blk = 0;
        int ncc = 0;
        bool use = false;
        // y-pass output mask (k_plan_rowmask): which 16-output chunks of each (column block, residue) hold a footprint row
        int yn2 = 0, yno = 0, yP = 0, yQ = 0;
        double yh = 0, ybtc = 0;
        DevBuf omask;
        int nblk = 0;
        double out_cells = 0;  // cells of C per transform the masked y-pass stores
    };
    std::vector<std::unique_ptr<ColPlan>> col_plans;
    std::vector<ColPlan *> col_plan_of[NCLS];  // [plan class][group * pairs + pair] of the current run
    ColPlan *column_plan(int pi, const Pair &pr, int fa, int fb, Nufft3<T> *n0) {
        const DimGeom &x = n0->geo.d[0], &y = n0->geo.d[1];
        const int w = n0->ker.w;
        const bool both = pr.herm || pr.mirror;
        for (auto &c : col_plans)
            if (c->serial == targets_serial && c->pair == pi && c->fa == fa && c->fb == fb && c->nos == x.nos() &&
                c->sP == x.sP() && c->cnt == x.cnt() && c->n2 == x.n2 && c->no == x.no && c->w == w && c->h == x.h &&
                c->btc == x.btc && c->both == both && c->yn2 == y.n2 && c->yno == y.no && c->yP == y.P && c->yQ == y.Q &&
                c->yh == y.h && c->ybtc == y.btc && c->yna == y.na && c->blk == n0->b_block_log_public())
                return c.get();
        std::unique_ptr<ColPlan> c(new ColPlan{targets_serial, pi, fa, fb, x.nos(), x.sP(), x.cnt(), x.n2, x.no, w, x.h, x.btc, both});
        const int nfg = fb - fa, stride = x.nos(), P = x.sP(), cnt = x.cnt();
        std::vector<int> tab((size_t)nfg * stride, 0);
        const int64_t nu = pr.h_ustart.empty() ? pr.n : (int64_t)pr.h_ustart.size() - 1;
        c->use = true;
        for (int fg = 0; fg < nfg && c->use; ++fg) {
            int *row = tab.data() + (size_t)fg * stride;
            const double sc = freqs[fa + fg];
            for (int64_t ui = 0; ui < nu; ++ui) {
                const int64_t kl = pr.h_ustart.empty() ? ui : pr.h_ustart[ui];
                const int64_t k = pr.h_idx[kl];
                const double sg = pr.h_flip[kl] ? -1.0 : 1.0;
                const double sv = sc * sg * (double)(T)h_bls[k];  // as k_interp forms it from the device copy
                const double th = x.h * (sv - sc * x.btc);
                for (int side = 0; side < (both ? 2 : 1); ++side) {
                    const double e = (side ? -1.0 : 1.0) * th * x.n2 * (0.5 / M_PI) + 0.5 * x.no;
                    const double t = e - 0.5 * w, jc = std::ceil(t);
                    const bool amb = jc - t < 1e-6 || jc - t > 1.0 - 1e-6;
                    int lo = std::max(0, std::min(x.no - w, (int)jc)), hi = lo + w - 1;
                    if (amb) {
                        lo = std::max(0, lo - 1);
                        hi = std::min(x.no - 1, hi + 1);
                    }
                    for (int i = lo; i <= hi; ++i) row[out_pos(i, P, cnt)] = 1;
                }
            }
            int run = 0;
            for (int i = 0; i < stride; ++i)
                if (row[i]) row[i] = ++run;
            c->ncc = std::max(c->ncc, run);
            if (run * 100 > x.no * 85) c->use = false;  // nothing to gain (decided on the first frequency already)
        }
        c->ncc = (c->ncc + 7) / 8 * 8;
        c->yn2 = y.n2; c->yno = y.no; c->yP = y.P; c->yQ = y.Q; c->yh = y.h; c->ybtc = y.btc;
        c->yna = y.na;
        c->blk = n0->b_block_log_public();
        if (c->use) {
            upload(c->tab, tab.data(), sizeof(int) * tab.size(), 0);
            c->h_tab = tab;
            // the x-pass stores compact column cc of a row at element (cc >> b) (na_y << b) + (cc & (2^b - 1)) of the row's
            // blocked output (RowDifArgs::out_blk): tabulated, so that a store index is one subtraction
            {
                std::vector<int> xt(tab.size());
                const int b = c->blk, rows = y.na << b, mask = (1 << b) - 1;
                for (size_t i = 0; i < tab.size(); ++i) xt[i] = tab[i] ? ((tab[i] - 1) >> b) * rows + ((tab[i] - 1) & mask) + 1 : 0;
                upload(c->xtab, xt.data(), sizeof(int) * xt.size(), 0);
            }
            // the y-pass output mask, on the device from the same targets
            if (y.logQ >= 9 && y.logQ <= 11 && !std::getenv("FFTVIS_HIP_NO_OUTPUT_MASK")) {
                const int bl = n0->ypass_cols_log(), nw = y.Q > 1024 ? y.Q / 1024 : 1;
                c->nblk = (c->ncc + (1 << bl) - 1) >> bl;
                const size_t words = (size_t)nfg * c->nblk * y.P * nw;
                c->omask.reserve(sizeof(unsigned long long) * words);
                FV_HIP(hipMemsetAsync(c->omask.p, 0, sizeof(unsigned long long) * words, stream));
                hipStream_t keep = n0->stream;
                n0->stream = stream;
                n0->build_rowmask(nu, d_bls.as<T>(), d_bls.as<T>() + nbls, pr.trivial ? nullptr : pr.idx->template as<int>(),
                                  pr.trivial ? nullptr : pr.flip->template as<signed char>(),
                                  pr.ustart ? pr.ustart->template as<int>() : nullptr, d_freqs.as<double>() + fa, nfg, both,
                                  c->tab.template as<int>(), c->ncc, c->omask.template as<unsigned long long>(), c->nblk, nw);
                n0->stream = keep;
                std::vector<unsigned long long> hm(words);
                FV_HIP(hipMemcpyAsync(hm.data(), c->omask.p, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, stream));
                FV_HIP(hipStreamSynchronize(stream));
                double bits = 0;
                for (unsigned long long v : hm) bits += __builtin_popcountll(v);
                c->out_cells = bits * 16.0 * (1 << bl) / nfg;
            }
        }
        col_plans.push_back(std::move(c));
        return col_plans.back().get();
    }

    // Direct y sums (fv_ydirect.h): the tables of one (frequency group, beam pair) for the geometry and column plan in
    // force.  The evaluation points -- every gather item's target and, packed runs, its mirror image -- are grouped by u
    // and then by v with the redundant-baseline tolerance (dedup_tol; compared with a cluster's first entry, so clusters
    // cannot drift), whatever FFTVIS_HIP_NO_TARGET_DEDUP says: the points, their groups and the decision below depend on
    // the geometry alone, and a run that gathers every baseline by itself maps its items to the same points.  A group's
    // first u fixes its footprint (origin and x-weights per frequency, placed as k_interp places them); its columns
    // are located through the column plan's table when one is armed, else through out_pos.  Contiguous groups form the
    // work ranges of k_ydirect: at most YD_NG groups, 1024 points and as many distinct column blocks as its LDS tile holds.
    // Inside a range every point is matched with the point of its group whose v is its negative (within the same
    // tolerance; each point in at most one pair) and the kernel walks slots, a pair or a single: FFTVIS_HIP_YD_PAIRS=0
    // (read per run) gives every point its own.  Points, map, statistics and the rule below do not know about slots.
    // Taken (use) when the points' (point, row) pairs are at most ydirect_gate() times the butterflies of the y-pass they
    // replace, columns x n2_y / 2 x log2 n2_y, on grids of the column plan's size class; FFTVIS_HIP_YDIRECT=1 takes it
    // wherever the tables can be built, 0 never.  Host arithmetic, once per (targets, group geometry); kept for later runs.
    struct YPlan {
        int64_t serial;
        int pair, fa, fb;
        const ColPlan *cp;
        int herm, blk, xp, w, pairing;
        int xn2, xno, xsP, xcnt, yna, yn2;
        double xh, xbtc, yh, ybtc;
        bool built = false, use = false;  // use: by the geometric rule (the switch is read per run)
        YdArgs a{};
        double cells = 0;  // cells of B per transform the sums read (mean over the frequencies)
        DevBuf wg, blkcnt, blkid, cref, xw, slv, slg, slp, map;
    };
    std::vector<std::unique_ptr<YPlan>> y_plans;
    std::vector<YPlan *> y_plan_of;  // [group * pairs + pair] of the current run (class 0)
    static double ydirect_gate() { return 1.0; }  // C3: 0.59 (taken); the same antennas scattered: about 2.3 (kept on the FFT y-pass)
    YPlan *ydirect_plan(int pi, const Pair &pr, int fa, int fb, Nufft3<T> *n0, const ColPlan *cp, bool forced) {
        const DimGeom &x = n0->geo.d[0], &y = n0->geo.d[1];
        const int w = n0->ker.w, blkB = n0->b_block_log_public(), blk = blkB ? blkB : 2;
        const int xp = (int)n0->b_pitch_with(cp && cp->use ? cp->ncc : 0);
        const char *epair = std::getenv("FFTVIS_HIP_YD_PAIRS");  // read per run: 0 gives every point a slot of its own
        const int pairing = epair && std::atoi(epair) == 0 ? 0 : 1;
        for (auto &c : y_plans)
            if (c->serial == targets_serial && c->pair == pi && c->fa == fa && c->fb == fb && c->cp == cp && c->herm == pr.herm &&
                c->blk == (blkB ? blkB : -2) && c->xp == xp && c->w == w && c->pairing == pairing && c->xn2 == x.n2 && c->xno == x.no && c->xsP == x.sP() &&
                c->xcnt == x.cnt() && c->yna == y.na && c->yn2 == y.n2 && c->xh == x.h && c->xbtc == x.btc && c->yh == y.h &&
                c->ybtc == y.btc)
                return c.get();
        std::unique_ptr<YPlan> c(new YPlan{targets_serial, pi, fa, fb, cp, pr.herm, blkB ? blkB : -2, xp, w, pairing, x.n2, x.no, x.sP(), x.cnt(),
                                           y.na, y.n2, x.h, x.btc, y.h, y.btc});
        y_plans.push_back(std::move(c));
        YPlan *yp = y_plans.back().get();
        const bool dbg = std::getenv("FFTVIS_HIP_DEBUG_YDIRECT") != nullptr;
        auto skip = [&](const char *why) {
            if (dbg) std::fprintf(stderr, "ydirect plan pair %d channels [%d, %d): not built: %s\n", pi, fa, fb, why);
            return yp;
        };
        const int nfg = fb - fa, BE = 1 << blk, sides = pr.herm ? 2 : 1;
        const int64_t N = !pr.h_upairs.empty() ? (int64_t)pr.h_upairs.size() / 2 : !pr.h_ustart.empty() ? (int64_t)pr.h_ustart.size() - 1 : pr.n;
        if (N == 0 || nfg == 0 || w > MAX_W || (pr.herm && (x.btc != 0.0 || y.btc != 0.0))) return skip("no items, or a packed run off centre");
        // the items' evaluation points
        const size_t NP = (size_t)N * sides;
        std::vector<double> pu(NP), pv(NP);
        for (int64_t i = 0; i < N; ++i) {
            const int64_t ui = !pr.h_upairs.empty() ? pr.h_upairs[2 * i] : i;
            const int64_t kl = pr.h_ustart.empty() ? ui : pr.h_ustart[ui];
            const int64_t k = pr.h_idx[kl];
            const double sg = pr.h_flip[kl] ? -1.0 : 1.0;
            for (int sd = 0; sd < sides; ++sd) {
                const double s2 = sd ? -sg : sg;
                pu[(size_t)i * sides + sd] = s2 * (double)(T)h_bls[k];
                pv[(size_t)i * sides + sd] = s2 * (double)(T)h_bls[(size_t)nbls + k];
            }
        }
        const double tol = std::max(dedup_tol(), 0.0);
        std::vector<int> ord(NP), grp(NP), map(2 * (size_t)N, 0);
        for (size_t i = 0; i < NP; ++i) ord[i] = (int)i;
        std::sort(ord.begin(), ord.end(), [&](int p, int q) { return pu[p] < pu[q] || (pu[p] == pu[q] && (pv[p] < pv[q] || (pv[p] == pv[q] && p < q))); });
        std::vector<double> gu;  // a group's u: its first entry's
        for (size_t i = 0; i < NP; ++i) {
            if (gu.empty() || pu[ord[i]] - gu.back() > tol) gu.push_back(pu[ord[i]]);
            grp[ord[i]] = (int)gu.size() - 1;
        }
        const int G = (int)gu.size();
        std::sort(ord.begin(), ord.end(), [&](int p, int q) { return grp[p] < grp[q] || (grp[p] == grp[q] && (pv[p] < pv[q] || (pv[p] == pv[q] && p < q))); });
        std::vector<double> ptv;
        std::vector<int> ptg, gstart(G + 1, 0);
        for (size_t i = 0; i < NP; ++i) {
            const int q = ord[i];
            if (ptv.empty() || ptg.back() != grp[q] || pv[q] - ptv.back() > tol) {
                ptv.push_back(pv[q]);
                ptg.push_back(grp[q]);
                ++gstart[grp[q] + 1];
            }
            map[(size_t)(q / sides) * 2 + (q % sides)] = (int)ptv.size() - 1;
        }
        for (int g = 0; g < G; ++g) gstart[g + 1] += gstart[g];
        const int64_t npts = (int64_t)ptv.size();
        // (the rule below cannot hold even if every group's columns are distinct: no tables)
        if (!forced && (double)npts * y.na > ydirect_gate() * ((double)G * w) * 0.5 * y.n2 * std::log2((double)y.n2)) return skip("too many points per u");
        if (blk < 2 || blk > 4) return skip("column blocks of fewer than 4 or more than 16 elements");
        if ((int64_t)y.na * xp >= ((int64_t)1 << 31)) return skip("a plane of B past the kernel's 32-bit cell offsets");
        // footprints per (frequency, group): compact (or stored) column of every footprint cell, x-weights
        const int P = x.sP(), cnt = x.cnt(), stride = x.nos(), ncols = n0->xcols_with(cp && cp->use ? cp->ncc : 0);
        const double beta = n0->ker.beta, c4 = n0->ker.c;
        std::vector<int> col((size_t)nfg * G * w);
        std::vector<double> xw((size_t)nfg * G * w);
        for (int fg = 0; fg < nfg; ++fg) {
            const double sc = freqs[fa + fg];
            for (int g = 0; g < G; ++g) {
                const double sv = sc * gu[g], th = x.h * (sv - sc * x.btc);
                const double e = th * x.n2 * (0.5 / M_PI) + 0.5 * x.no;
                const int j = std::max(0, std::min(x.no - w, (int)std::ceil(e - 0.5 * w)));
                for (int q = 0; q < w; ++q) {
                    const int pos = out_pos(std::min(j + q, x.no - 1), P, cnt);
                    int cc = pos;
                    if (cp && cp->use) {
                        const int t = cp->h_tab[(size_t)fg * stride + pos];
                        if (t == 0) return skip("a footprint column the column plan left out");  // (never met; the FFT y-pass then)
                        cc = t - 1;
                    }
                    if (cc < 0 || cc >= ncols || cc >= xp) return skip("a column outside B");
                    col[((size_t)fg * G + g) * w + q] = cc;
                    xw[((size_t)fg * G + g) * w + q] = es_eval<double>((double)(j + q) - e, beta, c4);
                }
            }
        }
        // work ranges: contiguous groups whose distinct blocks fit the tile at every frequency
        const int nbcap = yd_nbcap(blk);
        std::vector<int> wg;
        std::vector<std::vector<int>> cur(nfg), trial(nfg);
        auto blocks_with = [&](int g) {
            int worst = 0;
            for (int fg = 0; fg < nfg; ++fg) {
                trial[fg] = cur[fg];
                for (int q = 0; q < w; ++q) trial[fg].push_back(col[((size_t)fg * G + g) * w + q] >> blk);
                std::sort(trial[fg].begin(), trial[fg].end());
                trial[fg].erase(std::unique(trial[fg].begin(), trial[fg].end()), trial[fg].end());
                worst = std::max(worst, (int)trial[fg].size());
            }
            return worst;
        };
        std::vector<std::vector<int>> range_blocks;  // [range * nfg + fg]
        std::vector<double> slv;     // walk slots (fv_ydirect.h): base v,
        std::vector<int> slg, slp;   // group, (point at +theta, point at -theta or -1)
        int64_t npairs = 0;
        int g0 = 0;
        while (g0 < G) {
            for (auto &v : cur) v.clear();
            int ng = 0;
            while (g0 + ng < G && ng < YD_NG && gstart[g0 + ng + 1] - gstart[g0] <= YD_THREADS * YD_PTM) {
                if (blocks_with(g0 + ng) > nbcap) break;
                cur.swap(trial);
                ++ng;
            }
            if (ng == 0) return skip("one u-group alone does not fit a workgroup");
            // the range's walk slots, group by group: a group's points are sorted by v, so one index walks up from the
            // most negative and one down from the most positive; they pair when the two v cancel within the clustering
            // tolerance, else the one further from zero stays a single.  v = 0 pairs with nothing.
            const int s0 = (int)slv.size();
            for (int g = g0; g < g0 + ng; ++g) {
                auto single = [&](int p) {
                    slv.push_back(ptv[p]);
                    slg.push_back(g);
                    slp.insert(slp.end(), {p, -1});
                };
                int lo = gstart[g], hi = gstart[g + 1] - 1;
                while (lo <= hi) {
                    const double sum = ptv[lo] + ptv[hi];
                    if (pairing && lo < hi && ptv[lo] < 0.0 && ptv[hi] > 0.0 && std::fabs(sum) <= tol) {
                        slv.push_back(ptv[hi]);
                        slg.push_back(g);
                        slp.insert(slp.end(), {hi--, lo++});
                        ++npairs;
                    } else if (pairing && lo < hi && sum > 0.0) {
                        single(hi--);
                    } else {
                        single(lo++);
                    }
                }
            }
            wg.insert(wg.end(), {g0, ng, s0, (int)slv.size() - s0});
            for (int fg = 0; fg < nfg; ++fg) range_blocks.push_back(cur[fg]);
            g0 += ng;
        }
        const int nwg = (int)wg.size() / 4;
        std::vector<int> blkcnt((size_t)nfg * nwg), blkid((size_t)nfg * nwg * YD_NBMAX, 0), cref(col.size());
        double cells = 0;
        for (int r = 0; r < nwg; ++r)
            for (int fg = 0; fg < nfg; ++fg) {
                const std::vector<int> &bl = range_blocks[(size_t)r * nfg + fg];
                blkcnt[(size_t)fg * nwg + r] = (int)bl.size();
                cells += (double)bl.size() * BE * y.na / nfg;
                for (size_t i = 0; i < bl.size(); ++i) blkid[((size_t)fg * nwg + r) * YD_NBMAX + i] = bl[i];
                for (int g = wg[4 * r]; g < wg[4 * r] + wg[4 * r + 1]; ++g)
                    for (int q = 0; q < w; ++q) {
                        const int cc = col[((size_t)fg * G + g) * w + q];
                        const int slot = (int)(std::lower_bound(bl.begin(), bl.end(), cc >> blk) - bl.begin());
                        cref[((size_t)fg * G + g) * w + q] = (slot << 4) | (cc & (BE - 1));
                    }
            }
        upload(yp->wg, wg.data(), sizeof(int) * wg.size(), 0);
        upload(yp->blkcnt, blkcnt.data(), sizeof(int) * blkcnt.size(), 0);
        upload(yp->blkid, blkid.data(), sizeof(int) * blkid.size(), 0);
        upload(yp->cref, cref.data(), sizeof(int) * cref.size(), 0);
        upload(yp->xw, xw.data(), sizeof(double) * xw.size(), 0);
        upload(yp->slv, slv.data(), sizeof(double) * slv.size(), 0);
        upload(yp->slg, slg.data(), sizeof(int) * slg.size(), 0);
        upload(yp->slp, slp.data(), sizeof(int) * slp.size(), 0);
        upload(yp->map, map.data(), sizeof(int) * map.size(), 0);
        YdArgs &a = yp->a;
        a.w = w;
        a.nfg = nfg;
        a.nwg = nwg;
        a.ngroups = G;
        a.na_y = y.na;
        a.xp = xp;
        a.blk = blk;
        a.npts = npts;
        a.hy = y.h;
        a.btcy = y.btc;
        a.wg = yp->wg.template as<int>();
        a.blkcnt = yp->blkcnt.template as<int>();
        a.blkid = yp->blkid.template as<int>();
        a.cref = yp->cref.template as<int>();
        a.xw = yp->xw.template as<double>();
        a.slv = yp->slv.template as<double>();
        a.slg = yp->slg.template as<int>();
        a.slp = yp->slp.template as<int>();
        yp->cells = cells;
        yp->built = true;
        // the geometric rule: distinct columns read at the group's last frequency, whatever is stored
        std::vector<int> dc(col.begin() + (size_t)(nfg - 1) * G * w, col.end());
        std::sort(dc.begin(), dc.end());
        const double columns = (double)(std::unique(dc.begin(), dc.end()) - dc.begin());
        const double direct = (double)npts * y.na, ypass = columns * 0.5 * y.n2 * std::log2((double)y.n2);
        yp->use = n0->columns_possible() && n0->geo.cells_o() >= 4000000 && direct <= ydirect_gate() * ypass;
        if (dbg)
            std::fprintf(stderr, "ydirect plan pair %d channels [%d, %d): %lld items, %lld points on %d u-groups, %d work ranges, %.0f columns, "
                         "B cells read %.3g of %.3g needed, na_y %d, blocks of %d, plan %d, rule %.2f -> %s\n", pi, fa, fb, (long long)N,
                         (long long)npts, G, nwg, columns, cells, columns * y.na, y.na, BE, cp ? 1 : 0, direct / ypass, yp->use ? "taken" : "not taken");
        if (dbg)
            std::fprintf(stderr, "ydirect slots pair %d channels [%d, %d): %lld pairs, %lld singles, %lld walk slots for %lld points\n", pi, fa, fb,
                         (long long)npairs, (long long)(npts - 2 * npairs), (long long)slv.size(), (long long)npts);
        return yp;
    }

    // Eigenbeam mode (cpu_simulate.py:303-470): beams 0..K-1 are basis beams; every (k <= l) term
    // runs over ALL baselines without flips (:402-404) and is contracted with the coefficients.
    void set_basis(int nant, int K, int nfreq, const void *coefs, const int *ant1,
                   const int *ant2) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(polarized, "basis beams need a polarized engine (wrapper.py:280-283)");
        FV_REQUIRE(nbls > 0 && K >= 1 && K == (int)beams.size(), "set_array and the K basis beams first");
        FV_REQUIRE(nfreq == (int)freqs.size(), "beam_coefs frequency axis != freqs");
        for (int64_t b = 0; b < nbls; ++b)
            FV_REQUIRE(ant1[b] >= 0 && ant1[b] < nant && ant2[b] >= 0 && ant2[b] < nant, "antenna index out of range");
        nbasis = K;
        nant_basis = nant;
        {  // the coefficient gradient's reduction walks every antenna's baselines in this order: by baseline, first role first
            std::vector<int> start(nant + 1, 0), list((size_t)2 * nbls);
            for (int64_t b = 0; b < nbls; ++b) {
                ++start[ant1[b] + 1];
                ++start[ant2[b] + 1];
            }
            for (int a = 0; a < nant; ++a) start[a + 1] += start[a];
            std::vector<int> fill(start.begin(), start.end() - 1);
            for (int64_t b = 0; b < nbls; ++b) {
                list[fill[ant1[b]]++] = (int)(2 * b);
                list[fill[ant2[b]]++] = (int)(2 * b + 1);
            }
            upload(d_csr_start, start.data(), sizeof(int) * start.size(), 0);
            upload(d_csr, list.data(), sizeof(int) * list.size(), 0);
        }
        upload(d_coefs, coefs, sizeof(cplx<T>) * (size_t)nant * K * nfreq, 0);
        upload(d_ant1, ant1, sizeof(int) * nbls, 0);
        upload(d_ant2, ant2, sizeof(int) * nbls, 0);
        std::vector<int> bi, bj, idx(nbls);
        std::vector<int64_t> off(1, 0);
        std::vector<int> all;
        std::vector<signed char> fl;
        for (int k = 0; k < K; ++k)
            for (int l = k; l < K; ++l) {
                bi.push_back(k);
                bj.push_back(l);
                for (int64_t b = 0; b < nbls; ++b) {
                    all.push_back((int)b);
                    fl.push_back(0);
                }
                off.push_back((int64_t)all.size());
            }
        // (u, v) order here too: redundant baselines are gathered once (build_unique) and only the contraction with the
        // per-antenna coefficients runs per baseline
        set_beam_pairs((int)bi.size(), bi.data(), bj.data(), off.data(), all.data(), fl.data());
    }

    void set_chunking(int nchunks, double sb) override {
        FV_REQUIRE(nchunks >= 1, "nchunks must be >= 1");
        FV_REQUIRE(sb > 0.0 && sb <= 1.0, "source_buffer must be in (0, 1]");
        src_chunks = nchunks;
        source_buffer = sb;
    }

    // rotate -> horizon cut -> az/za -> 2 pi R topo for time ti; returns the device address of the
    // live above-horizon count (it never visits the host inside the loop).
    // The step works on the catalog range [s0, s0 + sn) (one source chunk); cap = capacity of the
    // compacted arrays; hslot = where the live count is kept for stats().
    const int *horizon_step(Lane &L, int ti, int64_t cap, int nblk, hipStream_t on, int64_t s0, int64_t sn,
                            int64_t hslot) {
        hipStream_t stream = on ? on : L.stream;
        DevBuf &d_blockcnt = L.d_blockcnt, &d_blockoff = L.d_blockoff, &d_scan_tot = L.d_scan_tot,
               &d_scan_off = L.d_scan_off, &d_xyz = L.d_xyz, &d_az = L.d_az, &d_za = L.d_za,
               &d_srcidx = L.d_srcidx;
        // R_t . eq on the fly, topocentric vectors the caller computed, or this time's astrometry context applied to the
        // chunk's sources first (into the lane's own (3, nsrc) scratch)
        const T *vec = ntimes_topo ? d_topo.as<T>() + (size_t)ti * 3 * nsrc : d_eq.as<T>();
        if (!astroms.empty()) {
            L.d_enu.reserve(sizeof(T) * 3 * (size_t)std::max<int64_t>(nsrc, 1));
            hipLaunchKernelGGL(k_astrom_topo<T>, dim3((unsigned)cdiv(sn, 256)), dim3(256), 0, stream, sn, nsrc, s0,
                               d_eq.as<T>(), astroms[ti], L.d_enu.template as<T>());
            vec = L.d_enu.template as<T>();
        }
        hipLaunchKernelGGL(k_horizon_count<T>, dim3(nblk), dim3(256), 0, stream, sn, nsrc, s0, vec,
                           rots[ti], d_blockcnt.as<int>());
        if (nblk <= 4096) {
            hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, stream,
                               d_blockcnt.as<int>(), d_blockoff.as<int>(), nblk);
        } else {
            const int nb2 = (int)cdiv(nblk, 1024);
            d_scan_tot.reserve(sizeof(int) * (nb2 + 1));
            d_scan_off.reserve(sizeof(int) * (nb2 + 1));
            hipLaunchKernelGGL(k_scan_blocks, dim3(nb2), dim3(1024), 0, stream,
                               d_blockcnt.as<int>(), d_blockoff.as<int>(), d_scan_tot.as<int>(), nblk);
            hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, stream,
                               d_scan_tot.as<int>(), d_scan_off.as<int>(), nb2);
            hipLaunchKernelGGL(k_scan_add, dim3(nb2), dim3(1024), 0, stream,
                               d_blockoff.as<int>(), d_scan_off.as<int>(), nblk);
        }
        hipLaunchKernelGGL(k_horizon_compact<T>, dim3(nblk), dim3(256), 0, stream, sn, nsrc, s0, vec,
                           rots[ti], rplane, d_blockoff.as<int>(), d_xyz.as<T>(), cap,
                           d_az.as<T>(), d_za.as<T>(), d_srcidx.as<int>(), d_err.as<int>() + 2);
        const int *Mp = d_blockoff.as<int>() + nblk;
        FV_HIP(hipMemcpyAsync(d_mhist.as<int>() + hslot, Mp, sizeof(int), hipMemcpyDeviceToDevice, stream));
        return Mp;
    }

    // Tight box of {2 pi R_plane v : |v| = 1, v_up >= 0} per coordinate.
    void source_box(double *xc, double *X) const {
        for (int d = 0; d < 3; ++d) {
            const double al = rplane.m[3 * d + 2];
            const double rad = std::sqrt(std::max(0.0, 1.0 - al * al));
            const double hi = al >= 0 ? 1.0 : rad, lo = al <= 0 ? -1.0 : -rad;
            xc[d] = 2.0 * M_PI * 0.5 * (hi + lo);
            X[d] = 2.0 * M_PI * 0.5 * (hi - lo) * (1.0 + 1e-9) + 1e-12;
        }
    }

    // Fine-grid cells per transform at sigma = 2 for channels [f0, f1): source box X, and in every dimension the largest
    // target box half-width over the pairs, box_B(p)[d] (the grid depends on the product of the two extents only, so the
    // adjoint, whose roles are swapped, sizes its grids from the same product).
    template <class BoxOf>
    double cells_at_sigma2(const double *X, int D, int f0, int f1, BoxOf box_B) const {
        const KerParams k2 = make_kernel(eps, 2.0);
        const double fmax = fmax_of(f0, f1);
        double cells2 = 1.0;
        for (int d = 0; d < D; ++d) {
            DimGeom g;
            g.X = X[d];
            double Bm = 0;
            for (const Pair &p : pairs) Bm = std::max(Bm, box_B(p)[d]);
            g.B = Bm;
            set_dim_geom(g, 2.0, k2.w, fmax, d == D - 1);
            cells2 *= g.n2;
        }
        return cells2;
    }
    // The "auto" upsampling factor (fv_sim_create upsampfac = 0) of a run whose grid has cells2 cells at sigma = 2 and
    // whose transforms spread and gather `points` points.
    double auto_sigma(double cells2, double points, int D) const {
        // accuracy floor of sigma = 1.25: the kernel transform falls by ~e^{-w/2} per dimension across
        // the band and rounding is amplified by that factor at band-edge targets -- ~1e-8 in fp64; in
        // fp32 it matches sigma = 2 down to eps = 1e-4 (HERA-350, top of the band: worst baseline
        // 5.8e-4 vs 9.9e-4, rel. l2 4.1e-5 vs 6.4e-5) and falls behind at 1e-5
        // (3-D: one more dimension of amplification -- 4e-8 seen at eps 2.5e-9 -- so ten times higher)
        const double eps_floor = (sizeof(T) == 8 ? 1e-8 : 1e-4) * (D == 3 ? 10.0 : 1.0);
        // measured (2-D): 8192^2 grids win with 1.25 from 1e5 sources (3.06 -> 1.57 s) up to 4e6 per
        // time step (31.1 -> 29.7 ms per 16-channel slice, ~30 cells per point); a 1024 x 512 grid
        // loses slightly even with 1e3 sources (its kernels are latency-bound, a smaller grid buys
        // little): so large grids only, and not when points outnumber the cells they save
        const double per_point = D == 2 ? 30.0 : 200.0;
        return eps >= eps_floor && cells2 >= 4.0e6 && cells2 >= per_point * points ? 1.25 : 2.0;
    }

    // Split [f0, f1) into groups of consecutive channels sharing one fine-grid geometry (sized
    // for the group's top frequency).  Small grids are launch-bound, so they tolerate a wide
    // frequency ratio (more wasted cells, far fewer launches); large grids are HBM-bound and get
    // a narrow one.  cells_top = fine-grid cells per transform at the highest frequency.
    std::vector<std::pair<int, int>> freq_groups(int f0, int f1, double cells_top, int tg) const {
        const char *er = std::getenv("FFTVIS_HIP_GROUP_RATIO");
        const char *eb = std::getenv("FFTVIS_HIP_GRID_BYTES");
        // grid bytes per launch, measured on C3: round 1 (four transforms per frequency) 3-4 GiB 350 ms per two
        // time steps, 8 GiB 362, 2 GiB 364, 1 GiB 369; round 2 (two per frequency, groups of whole eights):
        // 6 GiB 416.7 ms per four time steps (spread at 0.64 of the HBM roofline), 4 GiB 421.7 (0.54), 3 GiB 422.7
        const double budget = eb ? std::atof(eb) : 6.0 * 1024 * 1024 * 1024;
        const double fmax = fmax_of(f0, f1, 1.0);
        const double mb = cells_top * sizeof(cplx<T>) / (1024.0 * 1024.0);
        double ratio = 0.5 + 0.4 * std::min(1.0, std::max(0.0, std::log2(mb / 16.0) / 4.0));
        if (er) ratio = std::atof(er);
        std::vector<std::pair<int, int>> g;
        int a = f0;
        while (a < f1) {
            double lo = std::fabs(freqs[a]), hi = lo;
            int b = a + 1;
            while (b < f1) {
                const double nlo = std::min(lo, std::fabs(freqs[b])), nhi = std::max(hi, std::fabs(freqs[b]));
                if (nlo < ratio * nhi) break;
                const double sc = nhi / fmax;
                const double bytes = cells_top * sc * sc * (b + 1 - a) * tg * sizeof(cplx<T>);
                if (bytes > budget) break;
                lo = nlo;
                hi = nhi;
                ++b;
            }
            // whole spread chunks: a launch's transforms run as kernel launches of 16 / 8 / 4 / 2 / 1, and the
            // small ones re-walk the sources for few cells' worth of stores (14 transforms = 8 + 4 + 2: 0.52 of
            // the HBM roofline against 0.58 for 8 or 16); large grids therefore take groups of whole eights
            static const int quant = std::getenv("FFTVIS_HIP_GROUP_QUANT") ? std::atoi(std::getenv("FFTVIS_HIP_GROUP_QUANT")) : 8;
            const int cq = std::max(1, quant / std::max(tg, 1));  // channels per `quant` transforms
            if (quant > 1 && mb >= 64.0 && b - a > cq && b < f1) b = a + (b - a) / cq * cq;
            g.emplace_back(a, b);
            a = b;
        }
        return g;
    }

    // ---- host output, overlapped (reference cpu_simulate.py:843-854 returns a host array) ---------------------
    // A block of visibilities is 10 GB at C3.  Copied after the last kernel into fresh pageable memory it moves at
    // ~16 GB/s (first touch of every page included: 0.6 s after 1.6 s of compute).  Instead a helper thread pins
    // the caller's array in place (HostPin: parallel first touch, then hipHostRegister) while this thread queues the run,
    // every time step's last kernel records an event, and as soon as the array is pinned
    // the queueing thread issues, on a separate stream, one asynchronous copy per (channel, finished time step)
    // behind that step's event (53 GB/s, PCIe Gen5).  Only the last step's copy (0.5 GB, 10 ms) is left when the
    // kernels end.  FFTVIS_HIP_D2H_OVERLAP=0 or a block under 64 MiB keeps the single copy; so does a buffer the
    // driver refuses to pin.
    static size_t drain_min_bytes() {
        const char *e = std::getenv("FFTVIS_HIP_D2H_OVERLAP");
        if (e && std::atoi(e) == 0) return (size_t)-1;
        const char *m = std::getenv("FFTVIS_HIP_D2H_MIN_BYTES");
        return m ? (size_t)std::atof(m) : ((size_t)64 << 20);
    }
    hipEvent_t drain_event(size_t k) {
        while (drain_events.size() <= k) {
            hipEvent_t e;
            FV_HIP(hipEventCreateWithFlags(&e, std::getenv("FFTVIS_HIP_DEBUG_DRAIN") ? hipEventDefault : hipEventDisableTiming));
            drain_events.push_back(e);
        }
        return drain_events[k];
    }
    struct HostPin {
        std::thread th;
        std::atomic<int> state{0};  // 0 pinning, 1 pinned, -1 refused (locked-memory limit, exotic mapping)
        std::vector<std::pair<char *, size_t>> pieces;  // registered so far (helper thread only, until joined)
        double t_pinned = 0;  // seconds after start() (FFTVIS_HIP_DEBUG_DRAIN)
        hipStream_t *drain_on = nullptr;  // the stream copies into the pinned pieces are queued on (the owner's copy stream)
        std::chrono::steady_clock::time_point t0;
        double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
        // Pinning a FRESH array is slow because every page is touched for the first time inside the call, by one thread
        // (22 GB/s; 16.6 GB/s for a plain memset) -- the same pages touched by 16 threads first take 175-230 GB/s, and
        // registering touched memory 480 GB/s (measured, 4 GB).  So: a pool of threads writes one byte into every page
        // of the caller's array (its content is about to be overwritten by the block anyway), then the array is
        // registered in pieces cut at the multiples of 256 MiB of the address space (no page is registered twice; a copy
        // is split at the same addresses, drain_flush; short calls, so that a cold handle's allocations are not held up
        // behind the driver lock).  10 GB: pinned 0.08 s after the start instead of 0.45 s.
        static constexpr uintptr_t PIECE = (uintptr_t)256 << 20;
        static int touch_threads() {
            const unsigned hw = std::thread::hardware_concurrency();
            return (int)std::max(1u, std::min(16u, hw / 4));
        }
        void mark() { t0 = std::chrono::steady_clock::now(); }  // the clock of since() / t_pinned: the run's start
        // The destination is nseg runs of seg_bytes, seg_stride bytes apart (one run: a contiguous array; several: a
        // block inside a larger array, fv_sim_run_into).  shared: other processes write between and around the runs --
        // the first touch then only READS (a write could overwrite what another rank has already delivered; reading
        // faults a shared mapping's pages in just as well) and every run is registered on its own.
        void start(int device, void *ptr, size_t nseg, size_t seg_bytes, size_t seg_stride, bool shared, bool keep_clock = false) {
            if (!keep_clock) mark();
            if (nseg > 1 && seg_stride == seg_bytes) {
                seg_bytes *= nseg;
                nseg = 1;
            }
            th = std::thread([this, device, ptr, nseg, seg_bytes, seg_stride, shared] {
                (void)hipSetDevice(device);
                char *base = static_cast<char *>(ptr);
                {  // first touch, in parallel: thread i takes the i-th share of every run
                    const int nt = touch_threads();
                    std::vector<std::thread> pool;
                    const size_t share = (seg_bytes + nt - 1) / nt;
                    for (int i = 0; i < nt; ++i)
                        pool.emplace_back([=] {
                            for (size_t sg = 0; sg < nseg; ++sg) {
                                char *p = base + sg * seg_stride;
                                volatile char *q = p + std::min(seg_bytes, share * i);
                                volatile char *stop = p + std::min(seg_bytes, share * (i + 1));
                                if (shared) {
                                    char sink = 0;
                                    for (; q < stop; q += 4096) sink ^= *q;
                                    (void)sink;
                                } else {
                                    for (; q < stop; q += 4096) *q = 0;
                                }
                            }
                        });
                    for (std::thread &t : pool) t.join();
                }
                bool ok = true;
                // FFTVIS_HIP_PIN_FAIL_AFTER = n (tests): the (n + 1)-th registration is refused
                const char *ef = std::getenv("FFTVIS_HIP_PIN_FAIL_AFTER");
                const long fail_after = ef ? std::atol(ef) : -1;
                for (size_t sg = 0; ok && sg < nseg; ++sg) {
                char *p = base + sg * seg_stride, *end = p + seg_bytes;
                while (ok && p < end) {
                    const uintptr_t stop = (reinterpret_cast<uintptr_t>(p) / PIECE + 1) * PIECE;
                    char *q = std::min(end, reinterpret_cast<char *>(stop));
                    if ((fail_after < 0 || (long)pieces.size() < fail_after) &&
                        hipHostRegister(p, (size_t)(q - p), hipHostRegisterDefault) == hipSuccess) {
                        pieces.push_back({p, (size_t)(q - p)});
                        p = q;
                    } else {
                        (void)hipGetLastError();
                        ok = false;
                    }
                }
                }
                if (!ok) {
                    // refused part-way (locked-memory limit): the caller's array must not stay HALF pinned -- the fallback
                    // is ONE pageable copy over the whole range, and a range that is part registered, part pageable may be
                    // taken for pinned as a whole.  Nothing has been copied into the pieces yet (copies are only queued
                    // once state is 1), so they are simply released before the refusal is published.
                    for (auto &pc : pieces) (void)hipHostUnregister(pc.first);
                    pieces.clear();
                }
                t_pinned = since();
                state.store(ok ? 1 : -1, std::memory_order_release);
            });
        }
        bool pinned() const { return state.load(std::memory_order_acquire) == 1; }
        bool wait() {
            if (th.joinable()) th.join();
            return pinned();
        }
        ~HostPin() {  // also on the error paths: never leave the caller's memory pinned
            if (th.joinable()) th.join();
            // an exception may unwind past copies that are still in flight into the pieces: they end first
            if (!pieces.empty() && drain_on && *drain_on) (void)hipStreamSynchronize(*drain_on);
            for (auto &pc : pieces) (void)hipHostUnregister(pc.first);
        }
    };
    // The output block of a forward run, (nf, nt, tpol, nbls), on the device and zeroed: baselines not covered by any pair
    // stay zero (reference zero-initialises, :909-911).  At a host destination channel f of the block starts f * fs
    // elements after `out` (fv_sim_run_into's layout, consumed here).
    struct OutBlock {
        void *out;
        bool on_device;
        int nt, nf;
        cplx<T> *dout;
        int64_t per_tf, run, fs;  // elements per (frequency, time), per channel, between channels at the destination
        size_t bytes, run_bytes;
        bool shared;  // other processes write the rest of the destination array
        bool drain;   // the block leaves through the pinned caller array (drain_*)
    };
    OutBlock out_block(int nt, int nf, void *out, int out_on_device) {
        OutBlock o;
        o.out = out;
        o.on_device = out_on_device != 0;
        o.nt = nt;
        o.nf = nf;
        o.per_tf = (int64_t)tpol * nbls;
        o.run = (int64_t)nt * o.per_tf;
        o.fs = out_f_stride ? out_f_stride : o.run;
        o.shared = out_shared != 0;
        out_f_stride = 0;
        out_shared = 0;
        FV_REQUIRE(o.fs >= o.run, "fv_sim_run_into: the channel stride is shorter than a channel's run");
        o.bytes = sizeof(cplx<T>) * (size_t)nf * o.run;
        o.run_bytes = sizeof(cplx<T>) * (size_t)o.run;
        if (o.on_device) {
            o.dout = (cplx<T> *)out;
        } else {
            d_out.reserve(std::max<size_t>(o.bytes, 16));
            o.dout = d_out.as<cplx<T>>();
        }
        FV_HIP(hipMemsetAsync(o.dout, 0, o.bytes, stream));
        // (a block inside a larger array is pinned run by run: only worth it -- and only safe against two runs meeting in
        // one page -- when the runs are long)
        const bool pinnable = o.fs == o.run || (o.run_bytes >= ((size_t)1 << 20) && (size_t)(o.fs - o.run) * sizeof(cplx<T>) >= 8192);
        o.drain = !o.on_device && o.bytes >= drain_min_bytes() && pinnable;
        return o;
    }
    void pin_block(const OutBlock &o, HostPin &pin, bool keep_clock) {
        pin.start(device, o.out, (size_t)o.nf, o.run_bytes, sizeof(cplx<T>) * (size_t)o.fs, o.shared, keep_clock);
    }
    // the drained host output of a type-3 run: the pinning helper, the finished time steps and how many of them left
    struct Drain {
        HostPin pin;
        bool started = false;
        std::vector<DrainItem> items;
        size_t done = 0;
        const bool dbg = std::getenv("FFTVIS_HIP_DEBUG_DRAIN") != nullptr;
    };
    void pin_output(const OutBlock &o, Drain &dr) {
        pin_block(o, dr.pin, true);
        dr.started = true;
    }
    // queue the copies of the finished time steps dr.items[dr.done ...) behind their events
    void drain_flush(const OutBlock &o, Drain &dr) {
        if (!copy_stream) FV_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        cplx<T> *hout = static_cast<cplx<T> *>(o.out);
        for (; dr.done < dr.items.size(); ++dr.done) {
            const DrainItem &it = dr.items[dr.done];
            FV_HIP(hipStreamWaitEvent(copy_stream, it.ev, 0));
            for (int f = 0; f < o.nf; ++f)
                copy_block_pinned(hout + (int64_t)f * o.fs + (int64_t)it.t * o.per_tf, o.dout + ((int64_t)f * o.nt + it.t) * o.per_tf,
                                  sizeof(cplx<T>) * (size_t)it.n * o.per_tf, copy_stream);
        }
    }

    // one asynchronous copy of a whole block into a pinned caller array, split where the pinned pieces meet
    // the same for a block whose channels are o.fs elements apart at the destination: one run per channel
    void copy_block_to_host(const OutBlock &o, bool pinned, hipStream_t on) {
        if (o.fs == o.run) {
            if (pinned)
                copy_block_pinned(o.out, o.dout, o.bytes, on);
            else
                FV_HIP(hipMemcpyAsync(o.out, o.dout, o.bytes, hipMemcpyDeviceToHost, on));
            return;
        }
        if (!pinned) {
            FV_HIP(hipMemcpy2DAsync(o.out, sizeof(cplx<T>) * (size_t)o.fs, o.dout, o.run_bytes, o.run_bytes, (size_t)o.nf,
                                    hipMemcpyDeviceToHost, on));
            return;
        }
        for (int f = 0; f < o.nf; ++f)
            copy_block_pinned(static_cast<cplx<T> *>(o.out) + (int64_t)f * o.fs, o.dout + (int64_t)f * o.run, o.run_bytes, on);
    }
    // split where the pinned pieces meet (HostPin): a copy must lie inside one registration
    void copy_block_pinned(void *out, const void *dout, size_t bytes, hipStream_t on) {
        char *dst = static_cast<char *>(out);
        const char *src = static_cast<const char *>(dout);
        while (bytes) {
            const uintptr_t stop = (reinterpret_cast<uintptr_t>(dst) / HostPin::PIECE + 1) * HostPin::PIECE;
            const size_t n = std::min<size_t>(bytes, stop - reinterpret_cast<uintptr_t>(dst));
            FV_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, on));
            dst += n;
            src += n;
            bytes -= n;
        }
    }

    // ---- what the forward, type-1 and adjoint runs decide alike ----------------------------------------------------------
    void check_run(int t0, int t1, int f0, int f1) {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nsrc >= 0 && !rots.empty() && !freqs.empty() && nbls > 0 && !pairs.empty(),
                   "engine not fully configured");
        FV_REQUIRE(0 <= t0 && t0 <= t1 && t1 <= (int)rots.size(), "time range");
        FV_REQUIRE(0 <= f0 && f0 <= f1 && f1 <= (int)freqs.size(), "freq range");
        FV_REQUIRE((int)freqs.size() == nfreq_cat, "flux frequency axis != freqs");
        for (const Beam &b : beams) FV_REQUIRE(b.kind >= 0, "beam not set");
    }
    // largest |frequency| of channels [fa, fb), at least `lo`
    double fmax_of(int fa, int fb, double lo = 0.0) const {
        for (int f = fa; f < fb; ++f) lo = std::max(lo, std::fabs(freqs[f]));
        return lo;
    }
    // redundant baselines -> one gather target each (build_unique); the tolerance follows the engine's eps and the highest
    // frequency it knows (not the block's: blocks of a sharded run then agree on the runs)
    double dedup_tol() const { return 1e-3 * eps / (2.0 * M_PI * std::max(fmax_of(0, (int)freqs.size()), 1.0)); }
    // where polarisation product r of a baseline lands in a (frequency, time) slice of the output
    std::array<int64_t, 16> pol_offsets() const {
        std::array<int64_t, 16> po{};
        if (polarized)
            for (int r = 0; r < 4; ++r) po[r] = (int64_t)((r % 2) * 2 + r / 2) * nbls;
        return po;
    }
    // Source chunks (reference cpu_simulate.py:939): chunk c covers catalog sources [c csz, min(nsrc, (c + 1) csz)); the
    // compacted per-time arrays hold cap = source_buffer x csz sources.  Reserves those arrays in lanes [0, nl) and the
    // above-horizon count of every (time, chunk).
    struct Chunks {
        int n;
        int64_t csz, cap;
        int nblk;  // horizon-cut blocks of a chunk
    };
    Chunks source_chunks(int nl) {
        Chunks c;
        c.n = (int)std::max<int64_t>(1, std::min<int64_t>(src_chunks, nsrc));
        c.csz = std::max<int64_t>(cdiv(nsrc, c.n), 1);
        c.cap = std::max<int64_t>((int64_t)std::ceil(c.csz * source_buffer), 1);
        c.nblk = (int)cdiv(c.csz, 256);
        for (int li = 0; li < nl; ++li) {
            Lane &L = lanes[li];
            L.d_xyz.reserve(sizeof(T) * 3 * c.cap);
            L.d_az.reserve(sizeof(T) * c.cap);
            L.d_za.reserve(sizeof(T) * c.cap);
            L.d_srcidx.reserve(sizeof(int) * c.cap);
            L.d_blockcnt.reserve(sizeof(int) * (c.nblk + 1));
            L.d_blockoff.reserve(sizeof(int) * (c.nblk + 1));
        }
        reserve_mhist(sizeof(int) * rots.size() * std::max(1, src_chunks));
        return c;
    }

    // ---- what the type-1 run and the type-2 adjoint share: planes, frequency batches, the entry sort ----------------
    struct T1Plan {
        DimGeom g;     // n2 = P Q (na and no are the caller's: the two transforms prune opposite ends)
        int nb1;       // bins per dimension
        int nfb;       // frequencies per batch
        int64_t ecap;  // entry capacity of a batch
        int nbins;     // bins of a full batch
        int rec;       // bytes per entry record
    };
    // nf: channels the run walks; cap: slots of the compacted per-time arrays; images: the spread's periodic images
    // are entries too (the gather of the type-2 adjoint wraps its tile instead: exactly one entry per pair).
    T1Plan t1_plan(const KerParams &ker, double sigma, int nf, int64_t cap, bool images) const {
        T1Plan p;
        p.g.n1 = t1_nmodes;
        choose_pq(std::max((int)std::ceil(sigma * t1_nmodes), 2 * ker.w + 16), p.g);
        p.nb1 = (p.g.n2 + T1_PAD) >> BINLOG;
        // frequencies per batch: bounded by entries (~1.3 per (source, freq)) and by grid bytes
        const char *eb = std::getenv("FFTVIS_HIP_GRID_BYTES");
        const double budget = eb ? std::atof(eb) : 8.0 * 1024 * 1024 * 1024;
        const double plane_bytes = 2.0 * p.g.n2 * (double)p.g.n2 * tpol * sizeof(cplx<T>);
        // entries per live (source, frequency) pair: 1 + the periodic images of footprints that cross an
        // edge of the n2 x n2 plane -- (1 + (w + 1) / n2)^2 on average for uniformly placed sources (1.52
        // at w = 16 on the smallest, 64-cell planes); 5 % head-room on top, and a catalog that still
        // overflows (sources piled on a plane edge) fails the run (t1 overflow flag), never silently
        const double img = images ? (1.0 + (ker.w + 1.0) / p.g.n2) * (1.0 + (ker.w + 1.0) / p.g.n2) * 1.05 : 1.0;
        p.nfb = (int)std::max(1.0, std::min({(double)nf, budget / plane_bytes, 24.0e6 / (img * cap)}));
        p.ecap = (int64_t)(img * cap * p.nfb) + 4096;
        p.nbins = p.nfb * p.nb1 * p.nb1;
        p.rec = t1_record_bytes(ker.w, sizeof(T));
        return p;
    }
    // Counting sort of the (source, frequency) entries of one batch into 8 x 8-cell bins of their footprint origin, with
    // tabulated weights (k_t1_bin), on stream ps.  meta: 2 (nbins + 1) + 2 ints (counts, cursors), binstart: nbins + 1,
    // recs: a.ecap records; `scan` lends its scan buffers.
    template <bool IMG>
    void t1_sort(const T1Args &a, int nbins, const int *Mp, const T *xyz, DevBuf &meta, DevBuf &binstart, DevBuf &recs,
                 Nufft3<T> &scan, hipStream_t ps) {
        const KerParams &ker = scan.ker;
        const int nbn = a.nfg * a.nb1 * a.nb1;
        int *counts_p = meta.as<int>(), *cursor_p = counts_p + (nbins + 1), *ovf_p = d_err.as<int>() + 1;
        FV_HIP(hipMemsetAsync(meta.p, 0, sizeof(int) * (2 * (size_t)(nbins + 1) + 2), ps));
        const dim3 gb((unsigned)cdiv(a.cap * a.nfg, 256));
        hipLaunchKernelGGL((k_t1_bin<T, true, 0, IMG>), gb, dim3(256), 0, ps, a, Mp, xyz,
                           d_freqs.as<double>(), counts_p, (const int *)nullptr, cursor_p,
                           (unsigned char *)nullptr, (T)ker.beta, (T)ker.c, ovf_p);
        const hipStream_t own = scan.stream;
        scan.stream = ps;
        scan.exclusive_scan(counts_p, binstart.as<int>(), nbn);
        scan.stream = own;
        hipLaunchKernelGGL((ker.w == 9 ? k_t1_bin<T, false, 9, IMG> : ker.w == 5 ? k_t1_bin<T, false, 5, IMG> : ker.w == 7 ? k_t1_bin<T, false, 7, IMG> : k_t1_bin<T, false, 0, IMG>), gb, dim3(256), 0, ps, a, Mp,
                           xyz, d_freqs.as<double>(), counts_p, (const int *)binstart.as<int>(),
                           cursor_p, recs.as<unsigned char>(), (T)ker.beta, (T)ker.c, ovf_p);
    }

    // ---- type-1 run: per time, per frequency batch: bin (source, freq) entries on periodic
    // n2 x n2 planes, strengths, gather-spread, pruned FFT to the n_modes central modes, pick.
    void run_type1(int t0, int t1, int f0, int f1, const OutBlock &o) {
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = o.per_tf;
        // host output: the lattice path computes a C3 block in 65 ms, so the 10-GB copy IS the call -- the caller's array
        // is touched in parallel and pinned while the kernels run (HostPin), then one copy at PCIe rate (0.72 -> 0.3 s)
        HostPin pin;
        pin.drain_on = &stream;  // copy_block_pinned below rides on the main stream
        if (o.drain) pin_block(o, pin, false);
        const double sigma = this->sigma == 0.0 ? 2.0 : this->sigma;  // "auto" is a type-3 matter
        sigma_run = sigma;
        if (!t1fft) t1fft.reset(new Nufft3<T>(2, eps, sigma, stream));
        const KerParams &ker = t1fft->ker;
        const std::array<int64_t, 16> pol_off = pol_offsets();
        const Chunks ch = source_chunks(4);
        const int nch = ch.n;
        const int64_t csz = ch.csz, cap = ch.cap;
        // grid: n2 = P Q >= sigma n_modes (and >= 2 w), all n2 inputs live, n_modes + 1 outputs kept
        const T1Plan tp = t1_plan(ker, sigma, nf, cap, true);
        DimGeom g = tp.g;
        g.na = g.n2;
        g.no = t1_nmodes + 1;
        t1fft->set_fft_geometry(g, g);
        t1_dec.reserve(sizeof(T) * g.no);
        hipLaunchKernelGGL(k_deconv_table<T>, dim3(cdiv(g.no, 256)), dim3(256), 0, stream, g.no,
                           g.n2, ker, t1_dec.as<T>());
        const int nb1 = tp.nb1, nfb = tp.nfb, nbins = tp.nbins, rec = tp.rec;
        const int64_t ecap = tp.ecap;
        // Pipelined like the type-3 loop: the entry sort of unit (time, batch) u+1 (three kernels over
        // every (source, frequency) pair, ~25 % of a step) runs on the low-priority stream beside the
        // strengths / spread / FFT / pick of unit u; two sets of sort buffers and two sets of
        // per-time source arrays alternate.
        const char *ep = std::getenv("FFTVIS_HIP_PIPE");
        const int nunits = nt * nch * (int)cdiv(nf, nfb);
        const bool pipe = timing_level != 2 && nunits > 1 && !(ep && std::atoi(ep) == 0);
        const hipStream_t ps = pipe ? prep_stream : stream;
        for (int sset = 0; sset < (pipe ? 2 : 1); ++sset) {
            t1_meta[sset].reserve(sizeof(int) * (2 * (size_t)(nbins + 1) + 2));
            t1_binstart[sset].reserve(sizeof(int) * (nbins + 1));
            t1_rec[sset].reserve((size_t)rec * ecap);
        }
        t1_cs.reserve(sizeof(cplx<T>) * ecap * tpol);
        bool set_pending[2] = {false, false}, lane_pending[2] = {false, false};
        lane_mode = -1;  // a type-3 run after this one drains the streams before it reuses the lanes
        if (pipe) {  // the sort may start once the set-up queued on the main stream is done
            FV_HIP(hipEventRecord(ev_start, stream));
            FV_HIP(hipStreamWaitEvent(ps, ev_start, 0));
        }
        int unit = 0;

        for (int tc = 0; tc < nt * nch; ++tc) {  // (time, source chunk), chunks innermost (cpu_simulate.py:936-939)
            const int ti = t0 + tc / nch, chunk = tc % nch;
            const int64_t s0 = (int64_t)chunk * csz, sn = std::min<int64_t>(csz, nsrc - s0);
            if (nsrc == 0 || sn <= 0) continue;
            const int li = pipe ? tc % 2 : 0;
            Lane &L = lanes[li];
            DevBuf &d_xyz = L.d_xyz, &d_az = L.d_az, &d_za = L.d_za, &d_srcidx = L.d_srcidx;
            if (pipe && lane_pending[li]) FV_HIP(hipStreamWaitEvent(ps, L.done, 0));  // its strengths are done
            size_t e0 = ev_begin(TM_PREP, ps);
            const int *Mp = horizon_step(L, ti, cap, ch.nblk, ps, s0, sn, (int64_t)ti * nch + chunk);
            ev_end(e0, ps);
            mhist_log.push_back({ti * nch + chunk, 0.0});
            const size_t hist_slot = mhist_log.size() - 1;
            for (int fa = f0; fa < f1; fa += nfb, ++unit) {
                const int nfg = std::min(nfb, f1 - fa);
                const int ss = pipe ? unit % 2 : 0;
                DevBuf &meta = t1_meta[ss], &binstart = t1_binstart[ss], &recs = t1_rec[ss];
                T1Args a{};
                a.n2 = g.n2;
                a.nb1 = nb1;
                a.w = ker.w;
                a.nfg = nfg;
                a.f_first = fa;
                a.cap = cap;
                a.ecap = ecap;
                a.rec = rec;
                const int nbn = nfg * nb1 * nb1;
                if (pipe && set_pending[ss]) FV_HIP(hipStreamWaitEvent(ps, lanes[ss].heavy_done, 0));
                size_t e1 = ev_begin(TM_PREP, ps);
                t1_sort<true>(a, nbins, Mp, d_xyz.as<T>(), meta, binstart, recs, *t1fft, ps);
                ev_end(e1, ps);
                if (pipe) {
                    FV_HIP(hipEventRecord(lanes[ss].prep_done, ps));
                    FV_HIP(hipStreamWaitEvent(stream, lanes[ss].prep_done, 0));
                }
                const int *nent = binstart.as<int>() + nbn;
                for (const Pair &pr : pairs) {
                    if (pr.n == 0) continue;
                    size_t e2 = ev_begin(TM_STRENGTHS, stream);
                    StrengthArgs sa{};
                    sa.M = cap;
                    sa.nfg = nfg;
                    sa.f_first = fa;
                    sa.nfreq = nfreq_cat;
                    sa.polarized = polarized;
                    sa.pol_sky = pol_sky;
                    sa.same_beam = pr.bi == pr.bj;
                    // Hermitian packing: two planes per frequency instead of four for a single-beam pair
                    const bool herm1 = polarized && pr.bi == pr.bj && std::getenv("FFTVIS_HIP_NO_HERMITIAN") == nullptr;
                    const int tg = herm1 ? 2 : tpol;
                    sa.herm = herm1;
                    sa.dim = 2;
                    sa.bi = desc(pr.bi);
                    sa.bj = desc(pr.bj);
                    hipLaunchKernelGGL((beam_order == 3 ? k_t1_strengths<T, 3> : beam_order == 1 ? k_t1_strengths<T, 1> : k_t1_strengths<T, 0>),
                                       dim3(cdiv(ecap, 256)), dim3(256), 0, stream,
                                       sa, nent, ecap, (const unsigned char *)recs.as<unsigned char>(), rec,
                                       d_srcidx.as<int>(),
                                       d_az.as<T>(), d_za.as<T>(), d_flux.p, d_freqs.as<double>(),
                                       t1_cs.as<cplx<T>>());
                    ev_end(e2, stream);
                    const int nplanes = nfg * tg;
                    cplx<T> *A = t1fft->fft_input(nplanes);
                    size_t e3 = ev_begin(TM_SPREAD, stream);
                    const dim3 gs((unsigned)cdiv(g.n2 >> (BINLOG + 1), 4), (unsigned)(g.n2 >> (BINLOG + 1)), (unsigned)nfg);  // 16 x 16 cells per wave
                    // fp64: the accumulation on the matrix pipe (FFTVIS_HIP_T1_MM=0: the vector version)
                    static const bool t1_mm = !(std::getenv("FFTVIS_HIP_T1_MM") && std::atoi(std::getenv("FFTVIS_HIP_T1_MM")) == 0);
                    void (*kspread)(T1Args, const unsigned char *, const int *, const cplx<T> *, cplx<T> *) = nullptr;
                    if constexpr (sizeof(T) == 8)
                        if (t1_mm) kspread = herm1 ? k_t1_spread_mm<2> : polarized ? k_t1_spread_mm<4> : k_t1_spread_mm<1>;
                    if (!kspread) kspread = herm1 ? k_t1_spread<T, 2> : polarized ? k_t1_spread<T, 4> : k_t1_spread<T, 1>;
                    hipLaunchKernelGGL(kspread, gs, dim3(SPREAD_THREADS), 0, stream, a, (const unsigned char *)recs.as<unsigned char>(),
                                       (const int *)binstart.as<int>(), (const cplx<T> *)t1_cs.as<cplx<T>>(), A);
                    ev_end(e3, stream);
                    st[ST_SPREAD_LAUNCHES] += 1;
                    st[ST_SPREAD_CELLS] += (double)g.n2 * g.n2 * nplanes;
                    mhist_log[hist_slot].second += nplanes;
                    size_t e4 = ev_begin(TM_FFT, stream);
                    t1fft->fft(nplanes);
                    ev_end(e4, stream);
                    st[ST_FFT_CELLS] += ((double)g.n2 * g.n2 + 2.0 * g.no * g.n2 + (double)g.no * g.no) * nplanes;
                    size_t e5 = ev_begin(TM_INTERP, stream);
                    cplx<T> *obase = o.dout + ((int64_t)(fa - f0) * nt + (ti - t0)) * per_tf;
                    hipLaunchKernelGGL(k_t1_pick<T>, dim3(cdiv(pr.n * nfg, 256)), dim3(256), 0, stream,
                                       t1fft->fft_output(), g.no, g.P, g.cnt(), nfg, tg,
                                       (const int *)d_blint.as<int>(),
                                       (const int *)d_blint.as<int>() + nbls, pr.n,
                                       pr.trivial0 ? (const int *)nullptr : (const int *)(pr.idx0 ? pr.idx0 : pr.idx)->template as<int>(),
                                       pr.trivial0 ? (const signed char *)nullptr
                                                   : (const signed char *)(pr.flip0 ? pr.flip0 : pr.flip)->template as<signed char>(),
                                       (const T *)t1_dec.as<T>(), obase, (int64_t)nt * per_tf, pol_off[0],
                                       pol_off[1], pol_off[2], pol_off[3], chunk > 0, herm1, !reference_compat);
                    ev_end(e5, stream);
                    st[ST_GATHERED] += (double)pr.n * nplanes;
                    st[ST_N2X] = g.n2;
                    st[ST_N2Y] = g.n2;
                    st[ST_NA_XY] = g.n2 * 65536.0 + g.n2;
                    st[ST_W] = ker.w;
                }
                if (pipe) {
                    FV_HIP(hipEventRecord(lanes[ss].heavy_done, stream));
                    set_pending[ss] = true;
                }
            }
            if (pipe) {
                FV_HIP(hipEventRecord(L.done, stream));
                lane_pending[li] = true;
            }
        }
        if (!o.on_device) {
            copy_block_to_host(o, o.drain && pin.wait(), stream);
            FV_HIP(hipStreamSynchronize(stream));
            if (timing_level) ev_collect();
            check_errors();
        }
    }


    // ---- type-3 run ---------------------------------------------------------------------------------------------------
    // What a run decides, stage by stage (the functions below, in the order run() calls them); launch_strengths and the
    // unit loop read it.
    struct RunPlan {
        int t0, t1, f0, f1, nt, nf;
        double xc[3], X[3];  // box of the sources (source_box)
        int D = 2;           // dimensions of the transforms
        // height terms (height_terms, light_classes)
        int K = 0;  // terms (0: no expansion)
        double zc = 0.0, zh = 0.0, a = 0.0;
        int k0 = 0, k1 = 0;
        double eps_l[2] = {0.0, 0.0};
        int ncls = 1;  // plan classes in use (Lane::plan)
        // transforms per frequency on the grid (largest over the pairs), upsampling factor, grid-buffer cells per
        // transform at the top frequency, frequency groups (grid_and_groups)
        int tg_max = 1;
        double sigma = 2.0, cells_top = 1.0;
        std::vector<std::pair<int, int>> groups;
        // lane schedule (lane_schedule)
        int nlanes = 1, nlanes_used = 1;
        bool pipe = false, gang = false;
        Chunks ch{};
        // position adjoint (run_position_adjoint): every strengths launch writes three sets (k_strengths_moments) and
        // every (group, pair, term) runs three rounds of spread -> FFT -> gradient gather, one per set
        bool moments = false;
        // tangent (run_tangent): the gathers ADD into the output block with the tangent epilogue (k_interp<.., TANGENT>).
        // tan_w: device (6, nbls) fp64 by global baseline id -- rows 0-2 the weights of the three moments rounds
        // (R dbls / c), rows 3-5 the baselines' own vectors b' for the source rounds.  tan_sets: strength sets of the
        // source side (k_strengths_tangent), 1 + tan_D after the moments sets, or 0; tan_dtopo: device (nt, nsrc, 3) fp64.
        const double *tan_w = nullptr, *tan_dtopo = nullptr;
        int tan_sets = 0, tan_D = 0;
        double tan_h = 0.0;
        // basis tangent (run_basis_tangent): the gathers add, with the basis tangent epilogue (k_interp<.., BTAN>), into
        // bt_ndir copies of the output block, bt_stride elements apart, one per direction of bt_d: device
        // (bt_ndir, nant, K, nfreq) complex of this precision
        const void *bt_d = nullptr;
        int bt_ndir = 0;
        int64_t bt_stride = 0;
        bool forward = false;  // the plain forward run (run()): the only pass that may take the direct y sums
        int nsets() const { return (moments ? 3 : 0) + tan_sets; }  // strength sets per launch beyond the forward's one (0: the forward)
        // the plan class of height term kt: the run's own plan, or a light class's
        int cls(int kt) const { return k0 > 0 && kt >= k0 ? (kt >= k1 ? 2 : 1) : 0; }
    };

    void run(int t0, int t1, int f0, int f1, void *out, int out_on_device) override {
        check_run(t0, t1, f0, f1);
        if (mhist_log.size() > 65536) mhist_log.clear();  // nobody asked for the statistics of those runs
        const OutBlock o = out_block(t1 - t0, f1 - f0, out, out_on_device);
        if (type1) {
            run_type1(t0, t1, f0, f1, o);
            return;
        }
        // the helper touches and pins the caller's array once the first unit is queued: started at once, its sixteen page-
        // faulting threads slowed the main thread's set-up and first launches (first unit queued after 95 ms instead of 50)
        Drain dr;
        dr.pin.drain_on = &copy_stream;
        dr.pin.mark();
        static const bool pin_early = std::getenv("FFTVIS_HIP_PIN_EARLY") != nullptr;
        if (o.drain && pin_early) pin_output(o, dr);

        RunPlan r{t0, t1, f0, f1, t1 - t0, f1 - f0};
        r.forward = true;
        source_box(r.xc, r.X);
        height_terms(r);
        pair_setup(r);
        grid_and_groups(r);
        light_classes(r);
        lane_schedule(r);
        lane_plans(r);
        r.ch = source_chunks(r.nlanes_used);
        if (dr.dbg) std::fprintf(stderr, "run: set-up done %.3f s (lanes, unique targets, groups)\n", dr.pin.since());
        lane_buffers(r);
        if (dr.dbg) std::fprintf(stderr, "run: buffers and column plans %.3f s\n", dr.pin.since());
        queue_units(r, o, dr);
        finish_output(o, dr);
    }

    // ---- the row passes of a fit (DESIGN.md "Fused objective", "Gauss-Newton product", "Gains", "Jones gains") ------------
    // What the two passes share on the host.  An input of n values: the device array as it is, or the host array staged in
    // `buf` (null stays null).  An output: the device array, or `buf` reserved for it, copied back behind the kernels.
    template <typename X>
    const X *staged(DevBuf &buf, const FitIn &a, size_t n) {
        if (!a.p || a.on_device) return static_cast<const X *>(a.p);
        upload(buf, a.p, sizeof(X) * n, 0);
        return buf.as<X>();
    }
    template <typename X>
    X *staged_out(DevBuf &buf, const FitOut &a, size_t n) {
        if (!a.p || a.on_device) return static_cast<X *>(a.p);
        buf.reserve(std::max<size_t>(sizeof(X) * n, 16));
        return buf.as<X>();
    }
    void copy_back(const FitOut &a, const void *dev, size_t bytes) {
        if (a.p && !a.on_device) FV_HIP(hipMemcpyAsync(a.p, dev, bytes, hipMemcpyDeviceToHost, stream));
    }
    // The block of a pass: nrows = nf nt rows of L = tpol nbls values, n in all, and nx entries of the calibration (nfeed
    // nant gains or 4 nant matrix entries per row; gains and matrices need the pairs, matrices a polarized handle).
    struct FitBlock {
        int64_t nrows, L;
        size_t n, nx;
    };
    FitBlock fit_block(const char *entry, Cal kind, int t0, int t1, int f0, int f1) {
        check_run(t0, t1, f0, f1);
        FV_REQUIRE(kind != Cal::Jones || tpol == 4, std::string(entry) + ": Jones gains need a polarized handle");
        FV_REQUIRE(t1 > t0 && f1 > f0, std::string(entry) + ": empty range of times or frequencies");
        FV_REQUIRE(kind == Cal::None || gain_pairs.nbls == nbls, std::string(entry) + ": fv_sim_set_gain_pairs first (after the array is set)");
        const int64_t nrows = (int64_t)(f1 - f0) * (t1 - t0), L = (int64_t)tpol * nbls;
        return {nrows, L, (size_t)nrows * (size_t)L, (size_t)nrows * (size_t)cal_entries(kind, tpol, gain_pairs.nant)};
    }
    // The ending of every row pass: the rows' sums and the counters come back behind what the caller queued, with one
    // synchronisation; then the timers, the staged buffers' release, the run's error flags and the bad-input message.
    // The staged inputs of a pass belong to it: when together they exceed FFTVIS_HIP_ADJ_KEEP_BYTES (default 256 MiB) they
    // go back (fv_sim_run_adjoint's rule).  The set counted and given back: the data and the weights (for a weighting pass
    // too, so that what a handle holds afterwards does not depend on which of the two calls came last); with a calibration
    // its values and the gradient's block, for a weighting pass its direction; for Jones the rows' terms.
    void finish_rows(const RowScratch &rs, int64_t nrows, double *rows_host, Cal kind, bool weighting) {
        int hbad[2];
        collect_rows(stream, rs, nrows, rows_host, hbad);
        if (timing_level) ev_collect();
        std::vector<DevBuf *> set = {&d_res_d, &d_res_w};
        if (kind != Cal::None) set.insert(set.end(), {&d_res_g, &d_res_gg});
        if (kind != Cal::None && weighting) set.push_back(&d_res_dg);
        if (kind == Cal::Jones) set.push_back(&d_res_terms);
        size_t held = 0;
        for (const DevBuf *b : set) held += b->cap;
        const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
        if ((double)held > (ek ? std::atof(ek) : 256.0 * 1024 * 1024))
            for (DevBuf *b : set) b->release();
        check_errors();
        throw_if_bad_residual_input(hbad);
    }
    RowCal<T> row_cal(Cal kind, const cplx<T> *x, const cplx<T> *dx, cplx<double> *grad) {
        if (kind == Cal::None) return {};
        return {kind, &gain_pairs, x, dx, grad, kind == Cal::Jones ? d_res_terms.as<double>() : nullptr};
    }

    // The fused objective: gvis = 2 w (V - d) and chi2_ft = the (frequency, time) rows of sum w |V - d|^2, V this handle's
    // forward run of the block, which never leaves the device -- with gains or matrices, of the calibrated V', and grad the
    // gradient with respect to them.  run() fills the block on the device -- the caller's buffer, or d_out for a host
    // destination -- on whichever path the handle takes (type 1, type 3, basis beams, source chunks, height terms) and
    // leaves the main stream behind every lane; the row pass follows on it.  Host inputs are staged first; for Jones the
    // rows' terms take one more buffer, 8 bytes per value of the block.  One synchronisation at the end brings the rows'
    // sums, the bad-input counters and everything a host asked for.
    void residual_pass(Cal kind, int t0, int t1, int f0, int f1, const FitArrays &a, double *chi2_ft) override {
        static const char *const entry[] = {"fv_sim_run_residual", "fv_sim_run_residual_gains", "fv_sim_run_residual_jones"};
        const FitBlock b = fit_block(entry[(int)kind], kind, t0, t1, f0, f1);
        const cplx<T> *dd = staged<cplx<T>>(d_res_d, a.data, b.n);
        const T *dw = staged<T>(d_res_w, a.weights, b.n);
        const cplx<T> *dx = staged<cplx<T>>(d_res_g, a.x, b.nx);
        cplx<T> *dg = staged_out<cplx<T>>(d_out, a.gvis, b.n);
        cplx<double> *dgrad = staged_out<cplx<double>>(d_res_gg, a.grad, b.nx);
        const RowScratch rs = row_scratch<T>(d_res_sum, b.nrows, b.L);
        if (kind == Cal::Jones) d_res_terms.reserve(sizeof(double) * b.n);
        run(t0, t1, f0, f1, dg, 1);
        launch_residual<T>(stream, dg, dd, dw, b.nrows, b.L, rs, row_cal(kind, dx, nullptr, dgrad));
        copy_back(a.gvis, dg, sizeof(cplx<T>) * b.n);
        copy_back(a.grad, dgrad, sizeof(cplx<double>) * b.nx);
        finish_rows(rs, b.nrows, chi2_ft, kind, false);
    }
    // The Gauss-Newton product's weighting: the tangent blocks of [t0, t1) x [f0, f1) -- nparts device blocks in run()'s
    // layout, one per tangent pass of this handle -- become G, in place in parts_dev[0] (in vis_dev without parts), and q_ft
    // = the (frequency, time) rows of the weighted squares (launch_weight_rows); vis_dev is the forward block at the real
    // parameters, needed with a direction, with grad and without parts.  The kernels run on the main stream, which every
    // pass that filled a part has left behind its lanes.  Host inputs are staged first and given back under
    // residual_pass' rule.  One synchronisation at the end brings the rows' sums, the bad-weight counter and a host's grad.
    void weight_pass(Cal kind, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                     const FitArrays &a, double *q_ft) override {
        static const char *const entry[] = {"fv_sim_weight_block", "fv_sim_gain_weight_block", "fv_sim_jones_weight_block"};
        const FitBlock b = fit_block(entry[(int)kind], kind, t0, t1, f0, f1);
        const T *dw = staged<T>(d_res_w, a.weights, b.n);
        const cplx<T> *dx = staged<cplx<T>>(d_res_g, a.x, b.nx);
        const cplx<T> *ddx = staged<cplx<T>>(d_res_dg, a.dx, b.nx);
        cplx<double> *dgrad = staged_out<cplx<double>>(d_res_gg, a.grad, b.nx);
        cplx<T> *parts[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < nparts; ++j) parts[j] = static_cast<cplx<T> *>(parts_dev[j]);
        const RowScratch rs = row_scratch<T>(d_res_sum, b.nrows, b.L);
        if (kind == Cal::Jones) d_res_terms.reserve(sizeof(double) * b.n);
        launch_weight_rows<T>(stream, nparts, parts, static_cast<cplx<T> *>(vis_dev), dw, b.nrows, b.L, rs, row_cal(kind, dx, ddx, dgrad));
        copy_back(a.grad, dgrad, sizeof(cplx<double>) * b.nx);
        finish_rows(rs, b.nrows, q_ft, kind, true);
    }
    // The antenna pair of every baseline of the configured array, uploaded once with the incidence lists built from them.
    void set_gain_pairs(int nant, const int *ant1, const int *ant2) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nbls > 0, "fv_sim_set_gain_pairs: set the array first");
        gain_pairs.set(stream, nant, nbls, ant1, ant2);
    }

    // Height terms ("w-term expansion"): a non-coplanar array whose heights are small against the wavelength -- every
    // surveyed real array: centimetres to decimetres after the plane fit -- does not need a third grid dimension.
    // exp(i z s_z), z the sources' height coordinate in [zc - zh, zc + zh], s_z = nu b_z, is expanded in Chebyshev
    // polynomials of t = (z - zc) / zh (Jacobi - Anger: exp(i a t) = J_0(a) + 2 sum_k i^k J_k(a) T_k(t)):
    //     V(s) = sum_k  exp(i zc s_z) c_k(zh s_z)  F_k(s_x, s_y),   c_0 = J_0, c_k = 2 i^k J_k,   F_k = 2-D transform of c_j T_k(t_j),
    // K terms with 2 (a / 2)^K / K! <= eps / 10, a = zh max|s_z| (|J_k(a)| <= (a / 2)^k / k!): K 2-D transforms (7 for 3 cm of
    // scatter at 200 MHz; the Taylor series about zc this replaced needed a^K / K! <= eps / 10: 8) with all of the 2-D
    // machinery (Hermitian packing, column plan, source disc) instead of a 3-D grid whose third dimension is all kernel
    // width (16 planes for a source range of 1.4 cells) plus a z-pass.  The terms carry the transform's relative error
    // each, |T_k| <= 1, summed with weights |c_k| (sum <= 2 e^{a/2} - 1): the 2-D plans run at eps / (2 e^{a/2} - 1).
    // Taken while K <= 16 (|b_z| up to metres); beyond, or with FFTVIS_HIP_NO_WTERM=1, the 3-D transform runs.
    void height_terms(RunPlan &r) {
        if (!coplanar && !std::getenv("FFTVIS_HIP_NO_WTERM")) {
            double bz = 0;
            for (const Pair &p : pairs)
                if (p.n) bz = std::max(bz, p.Bs[2]);
            const double a = r.X[2] * fmax_of(r.f0, r.f1) * bz;  // largest |(z - zc) s_z|
            int K = 1;
            double term = a;  // 2 (a / 2)^K / K!: bound of the first neglected coefficient 2 |J_K|
            while (term > 0.1 * eps && K < 64) {
                ++K;
                term *= 0.5 * a / K;
            }
            const char *ek = std::getenv("FFTVIS_HIP_WTERM_MAX");
            if (K <= (ek ? std::atoi(ek) : 16)) {
                r.K = K;
                r.zc = r.xc[2];
                r.zh = r.X[2];
                r.a = a;
            }
        }
        r.D = r.K ? 2 : dim();
        st[ST_HEIGHT_TERMS] = r.K;
    }
    // Light terms: term k enters with weight |c_k| <= 2 (a / 2)^k / k!, so the higher terms need far less than the run's
    // tolerance -- with a = 0.35 (3 cm of scatter at 200 MHz) |c_2| = 0.03, |c_4| = 8e-5.  The terms k >= k0 run on a
    // second plan at eps_l = 0.3 eps / sum_{k >= k0} |c_k| and sigma = 1.25 (a grid of 0.39 x the cells: the FFT passes
    // are the bulk of a term), chosen as the smallest k0 whose tolerance is above that sigma's floor by a decade; fp64,
    // runs at sigma = 2 on large grids only.  k0 = 0: every term on the run's own plan.  FFTVIS_HIP_NO_WTERM_LIGHT=1.
    // Where the tail of the light terms can take a tolerance of 1e-4 or looser (a kernel of 8 cells instead of 12: the
    // gather of a light term is most of its time) the light terms split in two classes, [k0, k1) and [k1, K), with half
    // of the budget each; k1 = K: one class.
    void light_classes(RunPlan &r) {
        r.k0 = 0;
        r.k1 = r.K;
        if (r.K >= 3 && sizeof(T) == 8 && this->sigma == 2.0 && !std::getenv("FFTVIS_HIP_NO_WTERM_LIGHT")) {
            std::vector<double> ck(r.K);
            double c = 1.0;  // (a / 2)^k / k!
            for (int k = 0; k < r.K; ++k) {
                ck[k] = (k ? 2.0 : 1.0) * c;
                c *= 0.5 * r.a / (k + 1);
            }
            for (int k0 = 1; k0 + 2 <= r.K; ++k0) {  // at least two light terms
                double sl = 0;
                for (int k = k0; k < r.K; ++k) sl += ck[k];
                const double el = 0.3 * eps / sl;
                if (el >= 1e-7) {
                    r.k0 = k0;
                    r.eps_l[0] = std::min(el, 1e-2);
                    break;
                }
            }
            // a second class for the tail, where it can run at 1e-4 or looser: half of the light budget each
            if (r.k0 > 0 && !std::getenv("FFTVIS_HIP_WTERM_ONE_LIGHT_CLASS")) {
                for (int k1 = r.k0 + 1; k1 + 2 <= r.K; ++k1) {
                    double s2 = 0, s1 = 0;
                    for (int k = k1; k < r.K; ++k) s2 += ck[k];
                    for (int k = r.k0; k < k1; ++k) s1 += ck[k];
                    const double e2 = 0.15 * eps / s2, e1 = 0.15 * eps / s1;
                    if (e2 >= 1e-4 && e1 >= 1e-7) {
                        r.k1 = k1;
                        r.eps_l[0] = std::min(e1, 1e-2);
                        r.eps_l[1] = std::min(e2, 1e-2);
                        break;
                    }
                }
            }
        }
        // (sigma = 1.25 pays on large grids only, as in the automatic choice; FFTVIS_HIP_WTERM_LIGHT_CELLS moves the bound: tests)
        const char *elc = std::getenv("FFTVIS_HIP_WTERM_LIGHT_CELLS");
        if (r.k0 > 0 && r.cells_top < (elc ? std::atof(elc) : 4.0e6)) r.k0 = 0;
        if (r.k0 == 0) r.k1 = r.K;
        r.ncls = r.k0 == 0 ? 1 : r.k1 < r.K ? 3 : 2;
        st[ST_LIGHT_FROM] = r.k0;
        st[ST_LIGHTER_FROM] = r.k0 > 0 && r.k1 < r.K ? r.k1 : 0;
    }

    // Hermitian packing (k_interp<.., HERM>): a pair whose two beams are the same has Hermitian
    // strengths -- c_00, c_11 real, c_10 = conj(c_01) -- so two transforms per frequency (c_00 + i c_11,
    // c_01) evaluated at the baseline and at its mirror image give all four products: half the
    // spread, FFT and grid traffic of a polarized run.  The mirror targets need a box that is
    // symmetric about 0; taken when that box costs at most 1.5x the cells of the tight one and
    // the grid is large (small grids keep four transforms and the fused gather).  In eigenbeam mode the
    // diagonal (k, k) terms qualify.  FFTVIS_HIP_NO_HERMITIAN=1 turns it off.
    void pair_setup(RunPlan &r) {
        const bool herm_off = std::getenv("FFTVIS_HIP_NO_HERMITIAN") != nullptr;  // read per run: tests flip it
        const KerParams k2 = make_kernel(eps, 2.0);
        const double fmax = fmax_of(r.f0, r.f1);
        for (Pair &p : pairs) {
            p.herm = 0;
            if (!polarized || herm_off || p.n == 0) continue;
            // 1: same beam on both sides (Hermitian strengths; eigenbeams: the (k, k) terms);
            // 2: two different beams whose Jones matrices are real, unpolarized sky (all products real)
            const int mode = p.bi == p.bj ? 1 : (!pol_sky && beams[p.bi].real_valued && beams[p.bj].real_valued ? 2 : 0);
            if (!mode) continue;
            double cs = 1.0, ct = 1.0;
            for (int d = 0; d < r.D; ++d) {
                DimGeom gs, gt;
                gs.X = gt.X = r.X[d];
                gs.B = p.Bs[d];
                gt.B = p.B[d];
                set_dim_geom(gs, 2.0, k2.w, fmax, d == r.D - 1);
                set_dim_geom(gt, 2.0, k2.w, fmax, d == r.D - 1);
                cs *= gs.n2;
                ct *= gt.n2;
            }
            p.herm = cs >= 4.0e6 && cs <= 1.5 * ct ? mode : 0;
        }
        // reference_compat off, eigenbeams: an off-diagonal pair that is not packed gathers its (l, k) term
        // at -b: its targets need the symmetric box too
        for (Pair &p : pairs) p.mirror = nbasis && !reference_compat && p.bi != p.bj && !p.herm && p.n > 0;
        const double tol = dedup_tol();
        for (Pair &p : pairs) {
            build_unique(p, tol, r.K ? 2 : 3);
            pair_mirror_runs(p, tol);
        }
        for (const Pair &p : pairs)
            if (p.n) r.tg_max = std::max(r.tg_max, p.herm ? 2 : tpol);
    }

    // Upsampling factor "auto" (fv_sim_create upsampfac = 0): sigma = 1.25 shrinks the fine grid and
    // all FFT work by (2 / 1.25)^D at the price of a kernel 13-14 cells wide instead of 9 (every
    // source and target costs ~2x in 2-D), with NUFFT errors at or below sigma = 2's down to
    // eps ~ 1e-8 (fv_eskernel.h).  It pays when the FFT dominates: C3 (8192^2 cells, 1.1e5 points
    // per transform) 3.06 -> 1.57 s per step; C2 (1024 x 512, 5.7e3) would lose, 1.38 -> 1.58 ms.
    // Then the grid-buffer cells per transform at the top frequency, for the grouping heuristic, and the groups.
    void grid_and_groups(RunPlan &r) {
        r.sigma = this->sigma;
        if (r.sigma == 0.0) {
            int64_t nmax = 0;
            for (const Pair &p : pairs) nmax = std::max<int64_t>(nmax, p.n);
            const double cells2 = cells_at_sigma2(r.X, r.D, r.f0, r.f1, [](const Pair &p) { return p.box_B(); });
            r.sigma = auto_sigma(cells2, 0.5 * (double)nsrc + (double)nmax, r.D);
        }
        sigma_run = r.sigma;
        st[ST_SIGMA] = r.sigma;
        const KerParams k = make_kernel(eps, r.sigma);
        const double fmax = fmax_of(r.f0, r.f1);
        double na[3] = {1, 1, 1}, no[3] = {1, 1, 1};
        for (int d = 0; d < r.D; ++d) {
            DimGeom g;
            g.X = r.X[d];
            double Bm = 0;
            for (const Pair &p : pairs) Bm = std::max(Bm, p.box_B()[d]);
            g.B = Bm;
            set_dim_geom(g, r.sigma, k.w, fmax, d == r.D - 1);
            na[d] = g.na;
            no[d] = g.no;
        }
        r.cells_top = 2.0 * std::max({na[2] * na[1] * na[0], na[2] * na[1] * no[0], na[2] * no[0] * no[1], no[2] * no[0] * no[1]});
        r.groups = freq_groups(r.f0, r.f1, r.cells_top, r.tg_max);
    }

    // Two lanes always (two sets of per-time scratch and grid buffers; consecutive time steps alternate), memory
    // permitting.  Small grids (launch-bound) run them pipelined, see below.  Large grids (C3: 6 GiB of grid per
    // launch) run them FREELY on two streams of equal priority: the kernels of two time steps then share the
    // dispatcher like the kernels of two processes do -- a row pass of one step beside the spread or the gather of
    // the other, compute-bound waves beside memory-bound ones -- which is what two ranks on one GPU had over one
    // (843 against 883 ms per C3 step): 883 -> 844 ms in-process.  (With the second stream at a lower priority it
    // only ever filled the first one's tails: 868.)  Kernel durations measured in this mode are those of kernels
    // sharing the GPU.  FFTVIS_HIP_LANES=1: one stream.
    void lane_schedule(RunPlan &r) {
        int max_ntrans = 1;
        for (const auto &grp : r.groups) max_ntrans = std::max(max_ntrans, (grp.second - grp.first) * r.tg_max);
        const bool big_grids = r.cells_top * sizeof(cplx<T>) * max_ntrans > 1.5 * 1024 * 1024 * 1024;
        const char *el = std::getenv("FFTVIS_HIP_LANES");
        int nlanes = el ? std::atoi(el) : 2;
        if (!el && big_grids) {  // a second set of grid buffers must fit comfortably
            size_t mfree = 0, mtotal = 0;
            FV_HIP(hipMemGetInfo(&mfree, &mtotal));
            if (4.0 * r.cells_top * sizeof(cplx<T>) * max_ntrans > 0.5 * (double)mtotal) nlanes = 1;
        }
        const char *ep = std::getenv("FFTVIS_HIP_PIPE");
        const bool pipe_wanted = ep ? std::atoi(ep) != 0 : !big_grids;
        nlanes = std::max(1, std::min(pipe_wanted ? 2 : 4, std::min(nlanes, r.nt)));
        if (timing_level == 2) nlanes = 1;  // per-family event brackets only make sense on one stream
        r.nlanes = nlanes;
        // Two lanes, pipelined (default): every big kernel runs on the main (high-priority) stream,
        // one time step after the other, so kernel durations stay uncontended; the dozen tiny
        // latency-bound preparation kernels of step t+1 (rotation, horizon cut, bin sort, weight
        // tables) run on a low-priority stream beside step t's big kernels and fill their ramps
        // and tails.  FFTVIS_HIP_PIPE=0: the two lanes run freely on two streams instead.
        r.pipe = nlanes > 1 && pipe_wanted;
        // Gang mode (pipelined 2-D runs): two consecutive time steps share one launch each of the
        // spread and of every FFT pass (grid.y = 2: same geometry, their own sources and grids), which
        // halves the kernel boundaries per time step and doubles the workgroups that hide each other's
        // latency chains and tails.  Two pairs of lanes alternate, so that the preparation of the next
        // pair still runs beside this pair's big kernels.  FFTVIS_HIP_GANG=0 turns it off.
        const char *eg = std::getenv("FFTVIS_HIP_GANG");
        r.gang = r.pipe && r.D == 2 && r.nt >= 2 && timing_level != 2 && !(eg && std::atoi(eg) == 0);
        {  // forced direct y sums (FFTVIS_HIP_YDIRECT=1) run one time step per launch: they have no gang form
            const char *ey = std::getenv("FFTVIS_HIP_YDIRECT");
            if (ey && std::atoi(ey) == 1 && r.forward && sizeof(T) == 8 && !nbasis && !r.K) r.gang = false;
        }
        r.nlanes_used = r.gang ? 4 : nlanes;
        // Lane scratch outlives a run: with a device-side output buffer nothing synchronises between
        // two fv_sim_run calls, so the "last big kernels of this lane" events carry over (the next
        // run's first preparation waits for them) and the lane rotation continues where the previous
        // run stopped -- its first unit then takes the lanes that have been idle longest and prepares
        // beside the previous run's last big kernels.  A change of mode drains the streams instead.
        const int mode = r.gang ? 2 : r.pipe ? 1 : 0;
        st[ST_LANES] = nlanes;
        st[ST_LANE_MODE] = mode;
        if (mode != lane_mode) {
            FV_HIP(hipStreamSynchronize(stream));
            FV_HIP(hipStreamSynchronize(prep_stream));
            for (int li = 1; li < 4; ++li)
                if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
            for (Lane &L : lanes) L.heavy_pending = false;
            lane_mode = mode;
            lane_serial = 0;
        }
        if (nlanes > 2 && !r.pipe) {  // FFTVIS_HIP_LANES = 3 | 4: their streams, at the main stream's priority
            int prio_least = 0, prio_greatest = 0;
            FV_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
            for (int li = 2; li < nlanes; ++li)
                if (!lanes[li].stream || !lanes[li].own_stream) {
                    FV_HIP(hipStreamCreateWithPriority(&lanes[li].stream, hipStreamNonBlocking, prio_greatest));
                    lanes[li].own_stream = true;
                }
        }
    }

    // The type-3 plans of every lane in use, one per plan class (Lane::plan), made anew when their dimensions,
    // upsampling factor or tolerance change.
    void lane_plans(const RunPlan &r) {
        // height terms: term k enters with weight |c_k| <= 2 (a / 2)^k / k! (sum <= 2 e^{a/2} - 1), each with the
        // transform's relative error -- the run's own plan takes eps / (2 e^{a/2} - 1) so that the sum keeps eps
        const double eps_plan = r.K ? std::max(eps / (2.0 * std::exp(0.5 * r.a) - 1.0), sizeof(T) == 8 ? 1e-14 : 1e-7) : eps;
        for (int li = 0; li < r.nlanes_used; ++li) {
            Lane &L = lanes[li];
            for (int c = 0; c < r.ncls; ++c) {
                const int D = c ? 2 : r.D;
                const double e = c ? r.eps_l[c - 1] : eps_plan, sg = c ? 1.25 : r.sigma;
                std::unique_ptr<Nufft3<T>> &P = L.plan[c];
                if (!P || P->dim != D || P->sigma != sg || P->eps != e)
                    P.reset(new Nufft3<T>(D, e, sg, li < 2 || !r.pipe ? L.stream : stream));
                P->err_oob = d_err.as<int>();
                // the sources are 2 pi x (projections of unit vectors onto the array plane): inside a disc whatever the box
                P->disc_radius = (D == 2 || P->zdirect) && !std::getenv("FFTVIS_HIP_NO_DISC") ? 2.0 * M_PI : 0.0;
                P->transpose_flipped = !reference_compat;
                if (li > 0) P->order_cache = lanes[0].plan[c]->order_cache;  // one table per grid size for all lanes
                L.binned_ti[c] = -1;
            }
        }
    }

    // Size every lane's grid and strength buffers for the largest (frequency group, beam pair) of this run now,
    // before anything is queued (Nufft3::plan_buffer_cells): no reallocation -- a device synchronisation each --
    // while the first time step runs.  Then the column plans of every (class, group, pair), from the geometry the run
    // will set (large 2-D grids only).
    void lane_buffers(const RunPlan &r) {
        int64_t need_str = 0;
        for (const auto &grp : r.groups)
            for (const Pair &pr : pairs)
                if (pr.n) need_str = std::max<int64_t>(need_str, (grp.second - grp.first) * (pr.herm ? 2 : tpol));
        for (int c = 0; c < r.ncls; ++c) {  // the light height terms' plans have their own (smaller) grids
            Nufft3<T> *n0 = lanes[0].plan[c].get();
            int64_t need = 0;
            int na_max[3] = {8, 8, 8}, n2_max[3] = {64, 64, 64};
            for (const auto &grp : r.groups) {
                const double smax = fmax_of(grp.first, grp.second);
                for (const Pair &pr : pairs) {
                    if (pr.n == 0) continue;
                    const int ntrans = (grp.second - grp.first) * (pr.herm ? 2 : tpol);
                    for (double sl : {0.0, -1.0}) {  // with and without a column plan (its geometry takes no grid slack)
                        n0->grid_slack = sl;
                        need = std::max(need, n0->plan_buffer_cells(r.X, pr.box_B(), smax, na_max, n2_max) * ntrans);
                    }
                }
            }
            for (int li = 0; li < r.nlanes_used; ++li) {
                lanes[li].plan[c]->reserve_buffers(need, na_max, n2_max);
                lanes[li].plan[c]->strengths_buffer_reserve(r.ch.cap, (int)need_str * std::max(1, r.nsets()));
            }
        }
        for (auto &cpo : col_plan_of) cpo.assign(r.groups.size() * pairs.size(), nullptr);
        // plans of earlier target sets / groupings pile up in a long-lived handle: start over now and then (here,
        // before this run takes pointers into the list, and after everything an earlier run queued has finished)
        if (col_plans.size() > 512) {
            FV_HIP(hipDeviceSynchronize());
            col_plans.clear();
            y_plans.clear();  // (they point at column plans)
        }
        if (y_plans.size() > 512) {
            FV_HIP(hipDeviceSynchronize());
            y_plans.clear();
        }
        y_plan_of.assign(r.groups.size() * pairs.size(), nullptr);
        for (int c = 0; c < r.ncls; ++c) {
            if (std::getenv("FFTVIS_HIP_NO_COLUMN_PLAN")) break;
            Nufft3<T> *n0 = lanes[0].plan[c].get();
            if (n0->dim != 2 && !n0->zdirect) continue;
            for (size_t gi = 0; gi < r.groups.size(); ++gi) {
                const double smax = fmax_of(r.groups[gi].first, r.groups[gi].second);
                for (size_t pi = 0; pi < pairs.size(); ++pi) {
                    const Pair &pr = pairs[pi];
                    if (pr.n == 0) continue;
                    n0->grid_slack = 0.0;  // a plan's geometry: no grid slack (set_dim_geom)
                    n0->set_geometry(r.xc, r.X, pr.box_c(), pr.box_B(), smax);
                    if (!n0->columns_possible() || n0->geo.cells_o() < 4000000) continue;
                    col_plan_of[c][gi * pairs.size() + pi] = column_plan((int)pi, pr, r.groups[gi].first, r.groups[gi].second, n0);
                }
            }
            FV_HIP(hipStreamSynchronize(n0->stream));  // the table kernels of these set_geometry calls are done before the run's own
        }
        // direct y sums (ydirect_plan): forward runs of the run's own 2-D fp64 plan, one time step per launch; the tables
        // follow the geometry each (group, pair) will set -- a column plan's, or the plain one
        const char *ey = std::getenv("FFTVIS_HIP_YDIRECT");  // read per run: tests flip it
        const int ymode = ey ? std::atoi(ey) : -1;
        if (!r.forward || ymode == 0 || sizeof(T) != 8 || r.D != 2 || r.gang || nbasis || r.K || r.nsets()) return;
        Nufft3<T> *n0 = lanes[0].plan[0].get();
        size_t vals_need = 0;
        for (size_t gi = 0; gi < r.groups.size(); ++gi) {
            const int fa = r.groups[gi].first, fb = r.groups[gi].second;
            const double smax = fmax_of(fa, fb);
            for (size_t pi = 0; pi < pairs.size(); ++pi) {
                const Pair &pr = pairs[pi];
                const int tg = pr.herm ? 2 : tpol;
                if (pr.n == 0 || tg > 4 || pr.mirror) continue;
                const ColPlan *cp = col_plan_of[0][gi * pairs.size() + pi];
                if (cp && !cp->use) cp = nullptr;
                n0->grid_slack = cp ? 0.0 : -1.0;
                n0->set_geometry(r.xc, r.X, pr.box_c(), pr.box_B(), smax);
                if (ymode != 1 && (!n0->columns_possible() || n0->geo.cells_o() < 4000000)) continue;
                if (n0->fused_possible() && ymode != 1) continue;
                YPlan *yp = ydirect_plan((int)pi, pr, fa, fb, n0, cp, ymode == 1);
                if (!yp->built || !(ymode == 1 || yp->use)) continue;
                y_plan_of[gi * pairs.size() + pi] = yp;
                vals_need = std::max(vals_need, n0->yd_vals_bytes(yp->a.na_y, yp->a.nwg, fb - fa, tg, yp->a.npts));
                if (std::getenv("FFTVIS_HIP_DEBUG_YDIRECT")) {
                    int rps, ns;
                    n0->yd_slices(yp->a.na_y, yp->a.nwg, (fb - fa) * tg, yp->a.npts, rps, ns);
                    const int wgs = yp->a.nwg * (fb - fa) * tg * ns;
                    std::fprintf(stderr, "ydirect launch pair %d channels [%d, %d): %d slices of %d rows (na_y %d), %d workgroups, %d per round\n",
                                 (int)pi, fa, fb, ns, rps, yp->a.na_y, wgs, n0->yd_slot_count());
                }
            }
        }
        FV_HIP(hipStreamSynchronize(n0->stream));
        if (vals_need)
            for (int li = 0; li < r.nlanes_used; ++li) {
                lanes[li].plan[0]->yd_vals.reserve(vals_need);
                lanes[li].plan[0]->yd_slots = n0->yd_slots;  // one device: asked once
            }
    }

    // The unit loop: per (one or two time steps, source chunk) the per-time preparation, then per (frequency group, beam
    // pair, height term) strengths -> spread -> FFT -> gather.
    // gs != nullptr (the basis adjoint's coefficient pass, the position adjoint): o is the READ-ONLY G block and every
    // gather adds its inner products to the S buffer of its stream -- gs[0] when all big kernels share the main stream,
    // else the lane's.  r.moments (the position adjoint): three rounds per strengths launch, round d on strength set d
    // and into component d of S, (3, r.nf, nbls).
    // r.tan_w (the tangent): o is the pass's own output block, zeroed, and every round ADDS to it through the tangent
    // epilogue -- the three moments rounds with the weights of dbls when r.moments, then the r.tan_sets source rounds (the
    // beam term unweighted, set 1 + d with b'_d); no fused gather (it writes with atomics).
    void queue_units(const RunPlan &r, const OutBlock &o, Drain &dr, cplx<double> *const *gs = nullptr) {
        const int t0 = r.t0, t1 = r.t1, f0 = r.f0, nt = r.nt, D = r.D, nch = r.ch.n;
        const int64_t csz = r.ch.csz, cap = r.ch.cap;
        const bool pipe = r.pipe, gang = r.gang;
        const auto &groups = r.groups;
        const int64_t per_tf = o.per_tf;
        const std::array<int64_t, 16> pol_off = pol_offsets();
        if (r.nlanes > 1 && !pipe) {  // the other lanes start after the output memset queued on the main stream
            FV_HIP(hipEventRecord(ev_start, stream));
            for (int li = 1; li < r.nlanes; ++li) FV_HIP(hipStreamWaitEvent(lanes[li].stream, ev_start, 0));
        }

        const int sample_step = std::min(TIMING_STRIDE / 2, nt - 1);  // level-1 timing: this step of every 16
        const Pair *last_pair = nullptr;
        for (const Pair &pr : pairs)
            if (pr.n) last_pair = &pr;
        // only when every unit runs one geometry (one frequency group, one beam pair): with several, the
        // next preparation's set_geometry may rewrite the twiddle tables the FFT passes still read
        int active_pairs = 0;
        for (const Pair &pr : pairs) active_pairs += pr.n > 0;
        const char *erh = std::getenv("FFTVIS_HIP_RIDE_EVENT");
        const bool ride_heavy_done = !(erh && std::atoi(erh) == 0) && groups.size() == 1 && active_pairs == 1;
        for (int tnext = t0, ch = 0; tnext < t1;) {
            // units: (one or two time steps) x source chunk, chunks innermost (cpu_simulate.py:936-939)
            const int nm = gang && tnext + 1 < t1 ? 2 : 1;  // time steps in this unit
            const int tu = tnext;
            const int64_t s0 = (int64_t)ch * csz, sn = std::min<int64_t>(csz, nsrc - s0);
            const bool accumulate = ch > 0;  // later chunks add to the first one's visibilities (:1024,1069)
            const int chunk = ch;
            if (++ch == nch) {
                ch = 0;
                tnext += nm;
            }
            // host output: once the last chunk of these time steps is queued, an event marks them finished
            hipStream_t unit_stream = stream;  // where this unit's big kernels run (free-running lanes: the lane's own)
            auto close_time = [&]() {
                if (!o.drain || chunk != nch - 1) return;
                const hipEvent_t ev = drain_event(dr.items.size());
                // pipelined and single-lane runs: every big kernel is on `stream`; free-running lanes: all chunks of a time
                // step ran, in order, on its lane's stream -- the copy stream waits for THAT (the lanes never wait for
                // each other)
                FV_HIP(hipEventRecord(ev, unit_stream));
                dr.items.push_back({ev, tu - t0, nm});
                if (dr.pin.pinned()) drain_flush(o, dr);
            };
            if (nsrc == 0 || sn <= 0) {  // nothing above the horizon: the block stays zero (:945-946)
                close_time();
                continue;
            }
            const int64_t unit = lane_serial++;
            Lane *Ls[2];
            if (gang) {
                Ls[0] = &lanes[(unit % 2) * 2];
                Ls[1] = &lanes[(unit % 2) * 2 + 1];
            } else if (pipe) {
                Ls[0] = Ls[1] = &lanes[unit % r.nlanes];
            } else {
                // free-running lanes: the source chunks of one time step ADD to one another's visibilities, so they stay
                // on one stream, in order
                Ls[0] = Ls[1] = &lanes[tu % r.nlanes];
                unit_stream = Ls[0]->stream;
            }
            Lane &L0 = *Ls[0];
            const hipStream_t ls = pipe ? stream : L0.stream;        // big kernels
            const hipStream_t ps = pipe ? prep_stream : L0.stream;   // per-time preparation
            bool sampled = false, heavy_recorded = false;
            for (int m = 0; m < nm; ++m) sampled = sampled || (tu + m - t0) % TIMING_STRIDE == sample_step;
            // ---- per-time: rotate, horizon cut, az/za, 2 pi R topo --------------------------
            if (pipe && L0.heavy_pending) FV_HIP(hipStreamWaitEvent(ps, L0.heavy_done, 0));  // lane scratch is free
            const Pair *first_pair = nullptr;
            bool strengths_ahead = false;
            const int64_t M = cap;  // capacity: array stride and launch bound
            const int *Mps[2] = {nullptr, nullptr};
            size_t hist_slot[2] = {0, 0};
            size_t e0 = ev_begin(TM_PREP, ps);
            for (int m = 0; m < nm; ++m) {
                RoctxRange rr("prep");
                Lane &L = *Ls[m];
                Nufft3<T> *nufft = L.plan[0].get();
                nufft->stream = ps;
                Mps[m] = horizon_step(L, tu + m, cap, r.ch.nblk, ps, s0, sn, (int64_t)(tu + m) * nch + chunk);
                if (pipe) {  // the first (group, pair)'s bin sort belongs to the preparation as well
                    for (const Pair &pr : pairs) {
                        if (pr.n == 0 || groups.empty()) continue;
                        const ColPlan *cpq = col_plan_of[0][(size_t)(&pr - pairs.data())];  // group 0
                        nufft->grid_slack = cpq && cpq->use ? 0.0 : -1.0;
                        nufft->set_geometry(r.xc, r.X, pr.box_c(), pr.box_B(), fmax_of(groups[0].first, groups[0].second));
                        nufft->set_sources(M, L.d_xyz.template as<T>(), L.d_xyz.template as<T>() + cap,
                                           D > 2 ? L.d_xyz.template as<T>() + 2 * cap : nullptr, Mps[m]);
                        L.binned_ti[0] = (tu + m) * nch + chunk;
                        L.binned_serial[0] = nufft->geom_serial;
                        // ... and so do its strengths (beam x coherency, pre-phase): they depend on this
                        // step's sources only, not on the previous step's big kernels
                        launch_strengths(L, r, pr, groups[0].first, groups[0].second - groups[0].first, M, Mps[m], ps, 0, nullptr, tu + m);
                        first_pair = &pr;
                        strengths_ahead = true;
                        break;
                    }
                }
                hist_slot[m] = mhist_log.size();
                mhist_log.push_back({(tu + m) * nch + chunk, 0.0});
            }
            ev_end(e0, ps);
            if (pipe) {
                FV_HIP(hipEventRecord(L0.prep_done, ps));
                FV_HIP(hipStreamWaitEvent(ls, L0.prep_done, 0));
            }
            for (int m = 0; m < nm; ++m)
                for (int c = 0; c < r.ncls; ++c) Ls[m]->plan[c]->stream = ls;

            for (const auto &grp : groups) {
                const int fa = grp.first, fb = grp.second, nfg = fb - fa;
                const double smax = fmax_of(fa, fb);
                for (const Pair &pr : pairs) {
                    if (pr.n == 0) continue;
                    const int tg = pr.herm ? 2 : tpol;  // transforms per frequency on the grid
                    const int ntrans = nfg * tg;
                    // height terms (r.K): one round of strengths -> spread -> FFT -> gather per term, the gather adding
                    // term k with every baseline's own factor; otherwise a single round
                    for (int kt = 0; kt < std::max(1, r.K); ++kt) {
                    const int c = r.cls(kt);  // the plan of this term: the run's own, or a light class's
                    ColPlan *cp = col_plan_of[c][(size_t)(&grp - groups.data()) * pairs.size() + (size_t)(&pr - pairs.data())];
                    const bool on = cp && cp->use;
                    Nufft3<T> *nufft = L0.plan[c].get();
                    Nufft3<T> *mate = nm == 2 ? Ls[1]->plan[c].get() : nullptr;
                    for (int m = 0; m < nm; ++m) {
                        Lane &L = *Ls[m];
                        Nufft3<T> *nf_ = L.plan[c].get();
                        // ---- geometry + bin sort (skipped when unchanged since last set) -------
                        RoctxRange rr("prep");
                        size_t e1 = ev_begin(TM_PREP, ls);
                        nf_->grid_slack = on ? 0.0 : -1.0;
                        nf_->set_geometry(r.xc, r.X, pr.box_c(), pr.box_B(), smax);
                        if (L.binned_ti[c] != (tu + m) * nch + chunk || L.binned_serial[c] != nf_->geom_serial || nf_->M != M) {
                            nf_->set_sources(M, L.d_xyz.template as<T>(), L.d_xyz.template as<T>() + cap,
                                             D > 2 ? L.d_xyz.template as<T>() + 2 * cap : nullptr, Mps[m]);
                            L.binned_ti[c] = (tu + m) * nch + chunk;
                            L.binned_serial[c] = nf_->geom_serial;
                        }
                        ev_end(e1, ls);
                        // ---- strengths (already queued with the preparation for the first pair) -------
                        if (!(strengths_ahead && &grp == &groups.front() && &pr == first_pair && kt == 0))
                            launch_strengths(L, r, pr, fa, nfg, M, Mps[m], ls, kt, nf_, tu + m);
                    }
                    // ---- NUFFT ----------------------------------------------------------
                    const int nmom = r.moments ? 3 : 0;
                    const int nrounds = std::max(1, r.nsets());
                    // direct y sums for this (group, pair): lane_buffers decided (forward runs, the run's own plan)
                    YPlan *yp = c == 0 && !gs && !r.tan_w && nm == 1 && !y_plan_of.empty()
                                    ? y_plan_of[(size_t)(&grp - groups.data()) * pairs.size() + (size_t)(&pr - pairs.data())] : nullptr;
                    for (int rd = 0; rd < nrounds; ++rd) {
                    for (int m = 0; m < nm; ++m) {
                        Nufft3<T> *P = Ls[m]->plan[c].get();
                        P->strengths_off = r.nsets() ? (int64_t)rd * P->M * ntrans : 0;
                        P->arm_columns(on ? cp->tab.template as<int>() : nullptr, on ? cp->xtab.template as<int>() : nullptr, tg,
                                       on ? cp->ncc : 0, d_err.as<int>() + 3,
                                       on && cp->omask.p ? cp->omask.template as<unsigned long long>() : nullptr, on ? cp->nblk : 0);
                        P->col_out_cells = on && cp->omask.p ? cp->out_cells : 0.0;
                        P->arm_ydirect(yp ? &yp->a : nullptr, yp ? yp->map.template as<int>() : nullptr, yp ? yp->cells : 0.0,
                                       d_freqs.as<double>() + fa);
                    }
                    {
                    RoctxRange rr("spread");
                    if (timing_level >= 2 || (timing_level == 1 && sampled)) {  // 2 and 3: every launch
                        const size_t e3 = ev_slot(TM_SPREAD);
                        nufft->spread(ntrans, ev_pool[e3].a, ev_pool[e3].b, mate);
                        spread_timed += nm;  // a gang launch serves nm time steps: counted per time step
                    } else if (ride_heavy_done && pipe && &grp == &groups.back() && &pr == last_pair && kt + 1 >= std::max(1, r.K) &&
                               rd + 1 == nrounds) {
                        // the unit's last spread is the last reader of the lanes' per-time arrays (the FFT
                        // passes and the gather work on the grids): its dispatch carries the "lane scratch
                        // is free" event, which saves the main stream a marker packet per unit
                        nufft->spread(ntrans, nullptr, L0.heavy_done, mate);
                        heavy_recorded = true;
                    } else {
                        nufft->spread(ntrans, nullptr, nullptr, mate);
                    }
                    }
                    st[ST_SPREAD_LAUNCHES] += nm;  // launches are counted per (time, frequency group, beam pair)
                    st[ST_SPREAD_CELLS] += (double)nufft->spread_cells() * ntrans * nm;  // cells written (2-D: the blocks inside the source disc)
                    for (int m = 0; m < nm; ++m) mhist_log[hist_slot[m]].second += ntrans;
                    cplx<T> *obase = o.dout + ((int64_t)(fa - f0) * nt + (tu - t0)) * per_tf;
                    // small 2-D grids: the last FFT pass serves the targets from its LDS tiles (no C
                    // buffer, no gather kernel); the output block was zeroed at the start of the run
                    const bool fused =
                        !yp && !gs && !r.tan_w && !nbasis && !pr.herm && !r.K &&
                        nufft->prepare_fused_gather(pr.n, d_bls.as<T>(), d_bls.as<T>() + nbls,
                                                    pr.trivial ? nullptr : pr.idx->template as<int>(),
                                                    pr.trivial ? nullptr : pr.flip->template as<signed char>(),
                                                    d_freqs.as<double>() + fa, nfg, tpol, obase,
                                                    o.run, 1, pol_off.data(), targets_serial,
                                                    mate ? obase + per_tf : nullptr);
                    size_t e4 = ev_begin(TM_FFT, ls);
                    {
                        RoctxRange rr("fft");
                        nufft->fft(ntrans, mate);
                    }
                    ev_end(e4, ls);
                    st[ST_FFT_CELLS] += nufft->fft_traffic_cells() * ntrans * nm;
                    st[ST_FFT_FLOPS] += nufft->fft_flops() * ntrans * nm;
                    RoctxRange rg("gather");
                    size_t e5 = ev_begin(TM_INTERP, ls);
                    BasisTerm bt{d_coefs.p, d_ant1.as<int>(), d_ant2.as<int>(), pr.bi, pr.bj, nbasis,
                                 (int)freqs.size(), fa, 0, 0, nullptr, 0, 0, 0};
                    if (gs) {
                        if (!nbasis) bt.kk = bt.ll = 0;  // no basis term: the one inner product sum_r conj(G_r) V_r, slot 0
                        bt.gs = gs[pipe ? 0 : tu % r.nlanes] + (int64_t)rd * r.nf * nbls;  // (basis terms: one round)
                        bt.gs_nf = r.nf;
                        bt.gs_f0 = fa - f0;
                        bt.gs_nbls = nbls;
                        bt.gs_weighted = nbasis && r.moments;  // positions through basis beams: every term into round rd's block
                    }
                    if (r.bt_d) {
                        bt.dcoef = r.bt_d;
                        bt.ndir = r.bt_ndir;
                        bt.d_stride = (int64_t)nant_basis * nbasis * (int64_t)freqs.size();
                        bt.out_stride = r.bt_stride;
                    }
                    // exact eigenbeam symmetry (reference_compat off): the (l, k) term of an off-diagonal pair of
                    // complex basis beams comes from a second gather at -b (all-real pairs: packed, exact already)
                    const int nparts = nbasis && !reference_compat && pr.bi != pr.bj && !pr.herm ? 2 : 1;
                    const WTerm wterm{kt, r.zc, r.zh, (const void *)(d_bls.as<T>() + 2 * nbls)};
                    // tangent round rd: a moments round, the beam term's (no weights), or source set 1 + d with b'_d
                    const TanTerm tterm{rd < nmom ? r.tan_w + (int64_t)rd * nbls
                                                  : rd == nmom ? nullptr : r.tan_w + (int64_t)(3 + rd - nmom - 1) * nbls};
                    if (!fused)
                        for (int m = 0; m < nm; ++m)
                            for (int part = 1; part <= nparts; ++part) {
                                bt.part = nparts == 2 ? part : 0;
                                bt.negate = nparts == 2 && part == 2;
                                Ls[m]->plan[c]->interp(pr.n, d_bls.as<T>(), d_bls.as<T>() + nbls,
                                      D > 2 ? d_bls.as<T>() + 2 * nbls : nullptr,
                                      pr.trivial ? nullptr : pr.idx->template as<int>(),
                                      pr.trivial ? nullptr : pr.flip->template as<signed char>(),
                                      d_freqs.as<double>() + fa, nfg, tg, obase + (int64_t)m * per_tf,
                                      o.run, 1, pol_off.data(), accumulate || kt > 0, nbasis || gs ? &bt : nullptr, pr.herm,
                                      pr.ustart ? pr.ustart->template as<int>() : nullptr, pr.upairs ? pr.nitems : pr.nu,
                                      pr.upairs ? pr.upairs->template as<int>() : nullptr, r.K ? &wterm : nullptr,
                                      r.tan_w ? &tterm : nullptr);
                            }
                    ev_end(e5, ls);
                    for (int m = 0; m < nm; ++m) Ls[m]->plan[c]->strengths_off = 0;
                    st[ST_GATHERED] += (double)(pr.upairs ? pr.nitems : pr.ustart ? pr.nu : pr.n) * ntrans * nm * (pr.herm ? 2 : 1);  // footprints gathered: distinct targets; packed transforms are read at s and -s
                    if (c == 0) {  // (the run's own plan describes the run)
                        st[ST_N2X] = nufft->geo.d[0].n2;
                        st[ST_N2Y] = nufft->geo.d[1].n2;
                        st[ST_NA_XY] = nufft->geo.d[0].na * 65536.0 + nufft->geo.d[1].na;
                        st[ST_N2_3] = D > 2 ? nufft->geo.d[2].n2 : 1;
                        st[ST_NA_3] = D > 2 ? nufft->geo.d[2].na : 1;
                        st[ST_W] = nufft->ker.w;
                    }
                    }  // rounds
                    }  // height terms
                }
            }
            if (pipe) {
                if (!heavy_recorded) FV_HIP(hipEventRecord(L0.heavy_done, ls));
                L0.heavy_pending = true;
            }
            if (dr.dbg && tu == t0 && chunk == 0) std::fprintf(stderr, "run: first unit queued %.3f s\n", dr.pin.since());
            if (o.drain && !dr.started) pin_output(o, dr);
            close_time();
        }
        if (r.nlanes > 1 && !pipe) {  // join: everything queued on the main stream afterwards sees every lane
            for (int li = 1; li < r.nlanes; ++li) {
                FV_HIP(hipEventRecord(lanes[li].done, lanes[li].stream));
                FV_HIP(hipStreamWaitEvent(stream, lanes[li].done, 0));
            }
        }
    }

    // The end of a forward run with a host destination: the time steps not yet drained, or the whole block, leave for the
    // caller's array; the call returns synchronised.
    void finish_output(const OutBlock &o, Drain &dr) {
        if (o.on_device) return;
        if (o.drain && dr.pin.wait()) {
            const double t_queued = dr.pin.since();
            const size_t early = dr.done;
            drain_flush(o, dr);
            if (dr.dbg) {
                FV_HIP(hipStreamSynchronize(stream));
                std::fprintf(stderr, "drain: run queued %.3f s, pinned %.3f s, kernels done %.3f s, ", t_queued,
                             dr.pin.t_pinned, dr.pin.since());
            }
            FV_HIP(hipStreamSynchronize(copy_stream));
            FV_HIP(hipStreamSynchronize(stream));
            if (dr.dbg) {
                std::fprintf(stderr, "copies done %.3f s (%zu of %zu time-step items queued before the end)\n",
                             dr.pin.since(), early, dr.items.size());
                std::fprintf(stderr, "drain: time steps finished at [ms after the first]:");
                for (size_t i = 1; i < dr.items.size(); ++i) {
                    float ms = 0;
                    if (hipEventElapsedTime(&ms, dr.items[0].ev, dr.items[i].ev) == hipSuccess) std::fprintf(stderr, " %.0f", ms);
                }
                std::fprintf(stderr, "\n");
            }
        } else {
            copy_block_to_host(o, false, stream);
            FV_HIP(hipStreamSynchronize(stream));
        }
        if (timing_level) ev_collect();
        check_errors();
    }

    // ---- adjoint: gflux += A^T G, A = this handle's forward map (run) from fluxes to visibilities -------------------
    // One transposed slice per (time, frequency group, beam pair): k_adj_strengths folds the pair's baselines of the G
    // block onto its distinct vectors, a type-3 transform with the roles swapped takes them to the directions (2-D, or the
    // plain 3-D transform for non-coplanar arrays; lattice arrays take it too), k_adj_accumulate contracts with the beams.
    // Time steps alternate between the lanes (FFTVIS_HIP_LANES, 1 or 2), each with its own fp64 accumulator.
    void run_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux, int gflux_on_device,
                     int accumulate) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nbasis == 0, "the adjoint does not cover basis beams (set_basis / beam_coefs): fv_sim_run_basis_adjoint does");
        FV_REQUIRE(adjoint_path == 0 || type1,
                   "the type-2 adjoint (fv_sim_set_adjoint_path 1) needs a lattice handle (fv_sim_set_array_type1)");
        adjoint_flux(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, accumulate, adjoint_path == 1);
        last_adjoint_path = adjoint_path == 1 ? 2 : 3;
        adjoint_release();
        check_errors();
    }

    // Mode -> run table of a pair for the type-2 adjoint's fill: cell (my + na / 2) na + (mx + na / 2) of a plane lists the
    // runs (build_unique, three components) whose sign-adjusted integer vector is (mx, my) -- one per mode when the list
    // is visited in (u, v) order, one per member otherwise.  Counting sort in run order: the fill's sums have a fixed order.
    void mode_cells(Pair &p, int na) {
        if (p.n == 0 || (p.t2_cells && p.t2_serial == targets_serial && p.t2_na == na)) return;
        const int64_t nu = p.ustart ? p.nu : p.n;
        const size_t cells = (size_t)na * na;
        std::vector<int> tab(cells + 1 + (size_t)nu, 0), cell((size_t)nu);
        for (int64_t u = 0; u < nu; ++u) {
            const int64_t m = p.ustart ? p.h_ustart[u] : u;
            const double sg = p.h_flip[m] ? -1.0 : 1.0;
            const int mx = (int)std::lround(sg * h_bls[p.h_idx[m]]), my = (int)std::lround(sg * h_bls[(size_t)nbls + p.h_idx[m]]);
            FV_REQUIRE(std::abs(mx) < na / 2 && std::abs(my) < na / 2, "integer baseline outside the mode planes");
            cell[u] = (my + na / 2) * na + (mx + na / 2);
            ++tab[cell[u] + 1];
        }
        for (size_t c = 0; c < cells; ++c) tab[c + 1] += tab[c];
        std::vector<int> fill(tab.begin(), tab.begin() + cells);
        for (int64_t u = 0; u < nu; ++u) tab[cells + 1 + fill[cell[u]]++] = (int)u;
        p.t2_cells.reset(new DevBuf());
        upload(*p.t2_cells, tab.data(), sizeof(int) * tab.size(), 0);
        p.t2_serial = targets_serial;
        p.t2_na = na;
    }

    // The NUFFT sources of the transposed type-3 transforms (adjoint_flux, run_source_adjoint): per pair its runs' distinct
    // sign-adjusted vectors, (D, adj_np) on the device in p.adj_pos; exact basis form (reference_compat off): an
    // off-diagonal term's sources at b, then the same at -b.  Rebuilt when the targets or the count changed; both passes
    // go through here, so what one leaves is what the other expects.
    bool adj_mirrored(const Pair &p) const { return nbasis && !reference_compat && p.bi != p.bj; }
    void adj_sources(int D) {
        for (Pair &p : pairs) {
            const int64_t nu = p.ustart ? p.nu : p.n;
            const int64_t np = nu * (adj_mirrored(p) ? 2 : 1);
            if (p.n == 0 || (p.adj_pos && p.adj_serial == targets_serial && p.adj_np == np)) continue;
            std::vector<T> pos((size_t)D * np);
            for (int64_t u = 0; u < nu; ++u) {
                const int64_t m = p.ustart ? p.h_ustart[u] : u;
                const double sg = p.h_flip[m] ? -1.0 : 1.0;
                for (int d = 0; d < D; ++d) {
                    pos[(size_t)d * np + u] = (T)(sg * h_bls[(size_t)d * nbls + p.h_idx[m]]);
                    if (np > nu) pos[(size_t)d * np + nu + u] = -pos[(size_t)d * np + u];
                }
            }
            p.adj_pos.reset(new DevBuf());
            upload(*p.adj_pos, pos.data(), sizeof(T) * pos.size(), 0);
            p.adj_serial = targets_serial;
            p.adj_np = np;
        }
    }

    // The loop of run_adjoint.  Basis mode (run_basis_adjoint's flux pass): the pairs are the (k <= l) terms over all
    // baselines, the strengths carry every member's coefficient weights (k_adj_strengths_basis) and, in the exact form
    // (reference_compat off), an off-diagonal term has a second set of sources at -b.  Ends synchronised.
    // t2 (lattice handles, fv_sim_set_adjoint_path 1): the transpose of run_type1's slice instead of the swapped type-3
    // transform -- per (time, chunk, frequency batch) one entry sort without periodic images, per beam pair the runs'
    // strengths filled into the n_modes + 1 central modes (k_t2_fill), run_type1's planes transformed the other way
    // round (few inputs, all n2 outputs) and gathered at the entries (k_t2_gather).  Strengths, accumulators, channel
    // blocks, lanes and the reduction are the same code.
    void adjoint_flux(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux, int gflux_on_device,
                      int accumulate, bool t2 = false) {
        check_run(t0, t1, f0, f1);
        FV_REQUIRE(!t2 || (type1 && nbasis == 0), "the type-2 adjoint needs a lattice handle (fv_sim_set_array_type1)");
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        // whatever an earlier run queued (a device-output forward run leaves its lanes busy) is finished first: the lanes'
        // scratch is reused here; the next forward run starts its lane rotation afresh
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        if (copy_stream) FV_HIP(hipStreamSynchronize(copy_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        for (Lane &L : lanes) {
            L.heavy_pending = false;
            for (int &b : L.binned_ti) b = -1;
        }
        lane_mode = -1;
        // the forward's redundant-baseline runs, compared in all three components (a run's vector is its first member's)
        const double tol = dedup_tol();
        for (Pair &p : pairs) build_unique(p, tol, 3);
        const int D = dim();
        // box of the directions x = 2 pi R topo (R: the plane rotation, or the lattice basis^T of a type-1 array)
        double xc[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
        if (t2) {
            // no box: the planes are periodic
        } else if (type1) {
            for (int d = 0; d < 3; ++d) {
                const double *r = rplane.m + 3 * d;
                xc[d] = 0.0;
                X[d] = 2.0 * M_PI * std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * (1.0 + 1e-9) + 1e-300;
            }
        } else {
            source_box(xc, X);
        }
        auto adj_c = [&](const Pair &p) { return adj_mirrored(p) ? (const double *)zero3 : (const double *)p.btc; };
        auto adj_B = [&](const Pair &p) { return adj_mirrored(p) ? (const double *)p.Bs : (const double *)p.B; };
        if (t2) {
            for (Pair &p : pairs) p.adj_np = p.ustart ? p.nu : p.n;
        } else {
            adj_sources(D);
        }
        // the G block on the device
        const size_t g_bytes = sizeof(cplx<T>) * (size_t)nf * nt * per_tf;
        const cplx<T> *dg = (const cplx<T> *)gvis;
        if (!gvis_on_device) {
            upload(d_adj_g, gvis, g_bytes, 0);
            dg = d_adj_g.as<cplx<T>>();
        }
        // grid size (same product of extents as the forward's), upsampling factor and frequency groups
        // (the forward's rule for "auto", with the adjoint's own point count: its sources are the distinct vectors)
        int64_t nu_max = 1;
        for (const Pair &p : pairs) nu_max = std::max<int64_t>(nu_max, p.n ? p.adj_np : 0);
        // (t2: run_type1's factor -- "auto" is a type-3 matter -- and its frequency batches instead of groups)
        const double cells2 = t2 ? 0.0 : cells_at_sigma2(X, D, f0, f1, adj_B);
        const double sigma_a = this->sigma != 0.0 ? this->sigma : t2 ? 2.0 : auto_sigma(cells2, 0.5 * (double)nsrc + (double)nu_max, D);
        const double cells_top = 2.0 * cells2 * (sigma_a == 2.0 ? 1.0 : std::pow(1.25 / 2.0, D));
        const char *el = std::getenv("FFTVIS_HIP_LANES");
        const int nlanes = std::max(1, std::min(2, std::min(el ? std::atoi(el) : 2, std::max(nt, 1))));
        const Chunks sc = source_chunks(nlanes);
        const int nch = sc.n;
        const int64_t csz = sc.csz, cap = sc.cap;
        const int comps = pol_sky ? 8 : 1;
        // Channel blocks: a lane's accumulator holds nsrc x (channels of a block) x comps doubles, at most
        // FFTVIS_HIP_ADJ_ACC_BYTES (default 256 MiB); every block walks the time steps once and is reduced into gflux.
        const char *eab = std::getenv("FFTVIS_HIP_ADJ_ACC_BYTES");
        const double acc_max = eab ? std::atof(eab) : 256.0 * 1024 * 1024;
        const int nfb = (int)std::max<double>(1.0, std::min<double>(nf, std::floor(acc_max / (8.0 * comps * std::max<int64_t>(nsrc, 1)))));
        // t2: the lanes' FFT plans (their kernel parameters size the entry records), run_type1's planes with the pruned
        // ends swapped -- na = n_modes + 1 inputs in whole 8-cell units, every one of the n2 outputs kept -- and its batches
        T1Plan tp{};
        DimGeom g2;
        if (t2) {
            for (int li = 0; li < nlanes; ++li) {
                Lane &L = lanes[li];
                if (!L.adj2 || L.adj2->sigma != sigma_a || L.adj2->eps != eps) L.adj2.reset(new Nufft3<T>(2, eps, sigma_a, L.stream));
                L.adj2->stream = L.stream;
            }
            tp = t1_plan(lanes[0].adj2->ker, sigma_a, std::min(nf, nfb), cap, false);
            g2 = tp.g;
            g2.na = (int)cdiv(t1_nmodes + 1, 1 << BINLOG) << BINLOG;
            g2.no = g2.n2;
            FV_REQUIRE(g2.na <= g2.n2, "type-2 adjoint: more modes than grid cells");
            for (Pair &p : pairs) mode_cells(p, g2.na);
        }
        struct FBlock {
            int b0, b1;
            std::vector<std::pair<int, int>> groups;
        };
        std::vector<FBlock> fblocks;
        int nfg_max = 1;
        for (int b0 = f0; b0 < f1; b0 += nfb) {
            FBlock fb{b0, std::min(f1, b0 + nfb), {}};
            if (t2) {
                for (int fa = fb.b0; fa < fb.b1; fa += tp.nfb) fb.groups.push_back({fa, std::min(fb.b1, fa + tp.nfb)});
            } else {
                fb.groups = freq_groups(fb.b0, fb.b1, cells_top, tpol);
            }
            for (const auto &grp : fb.groups) nfg_max = std::max(nfg_max, grp.second - grp.first);
            fblocks.push_back(std::move(fb));
        }
        const size_t acc_bytes = sizeof(double) * (size_t)std::max<int64_t>(nsrc * std::min(nf, nfb) * comps, 1);
        for (int li = 0; li < nlanes; ++li) {
            Lane &L = lanes[li];
            if (t2) {
                L.adj2->set_fft_geometry(g2, g2);
                L.d_t2_dec.reserve(sizeof(T) * g2.na);
                hipLaunchKernelGGL(k_deconv_table<T>, dim3(cdiv(g2.na, 256)), dim3(256), 0, L.stream, g2.na, g2.n2, L.adj2->ker,
                                   L.d_t2_dec.template as<T>());
                L.d_t2_meta.reserve(sizeof(int) * (2 * (size_t)(tp.nbins + 1) + 2));
                L.d_t2_binstart.reserve(sizeof(int) * (tp.nbins + 1));
                L.d_t2_rec.reserve((size_t)tp.rec * tp.ecap);
            } else {
                if (!L.adj || L.adj->dim != D || L.adj->sigma != sigma_a || L.adj->eps != eps)
                    L.adj.reset(new Nufft3<T>(D, eps, sigma_a, L.stream));
                L.adj->stream = L.stream;
                L.adj->err_oob = d_err.as<int>();
                L.adj->disc_radius = 0.0;  // its sources are baselines
                L.adj->transpose_flipped = false;
                L.adj->arm_columns(nullptr, nullptr, tpol, 0);
            }
            L.d_adj_q.reserve(sizeof(cplx<T>) * (size_t)nu_max * nfg_max * tpol);
            L.d_adj_z.reserve(sizeof(cplx<T>) * (size_t)cap * nfg_max * tpol);
            L.d_adj_acc.reserve(acc_bytes);
        }
        // gflux on the device, zeroed or holding what the call adds to (main stream: before every reduction)
        const size_t gf_bytes = sizeof(T) * (size_t)nsrc * nfreq_cat * comps;
        T *dgf = (T *)gflux;
        if (!gflux_on_device) {
            d_adj_gf.reserve(std::max<size_t>(gf_bytes, 16));
            dgf = d_adj_gf.as<T>();
            if (accumulate && gf_bytes) FV_HIP(hipMemcpyAsync(dgf, gflux, gf_bytes, hipMemcpyHostToDevice, stream));
        }
        if (!accumulate && gf_bytes) FV_HIP(hipMemsetAsync(dgf, 0, gf_bytes, stream));
        const std::array<int64_t, 16> pol_off = pol_offsets();  // the forward's output slots
        int64_t z_off[16] = {0};
        for (int r = 0; r < tpol; ++r) z_off[r] = (int64_t)r * cap;
        const int ord = beam_order == 3 ? 3 : beam_order == 1 ? 1 : 0;
        for (size_t bi = 0; bi < fblocks.size(); ++bi) {
            const FBlock &fb = fblocks[bi];
            const int nfa = fb.b1 - fb.b0;
            for (int li = 0; li < nlanes; ++li) {
                if (bi > 0) {  // the previous block's reduction has read this accumulator
                    FV_HIP(hipEventRecord(ev_start, stream));
                    FV_HIP(hipStreamWaitEvent(lanes[li].stream, ev_start, 0));
                }
                FV_HIP(hipMemsetAsync(lanes[li].d_adj_acc.p, 0, sizeof(double) * (size_t)std::max<int64_t>(nsrc * nfa * comps, 1),
                                      lanes[li].stream));
            }
            for (int t = t0; t < t1; ++t) {
                Lane &L = lanes[(t - t0) % nlanes];
                const hipStream_t ls = L.stream;
                Nufft3<T> &P = t2 ? *L.adj2 : *L.adj;
                for (int ch = 0; ch < nch; ++ch) {
                    const int64_t s0 = (int64_t)ch * csz, sn = std::min<int64_t>(csz, nsrc - s0);
                    if (nsrc == 0 || sn <= 0) continue;  // nothing above the horizon: nothing to add
                    const int *Mp = horizon_step(L, t, cap, sc.nblk, ls, s0, sn, (int64_t)t * nch + ch);
                    const T *xyz = L.d_xyz.template as<T>();
                    for (const auto &grp : fb.groups) {
                        const int fa = grp.first, nfg = grp.second - grp.first;
                        const double smax = fmax_of(fa, grp.second);
                        T1Args ta{};
                        if (t2) {  // the batch's (source, channel) entries in bin order, one each, for every pair
                            ta.n2 = g2.n2;
                            ta.nb1 = tp.nb1;
                            ta.w = P.ker.w;
                            ta.nfg = nfg;
                            ta.f_first = fa;
                            ta.cap = cap;
                            ta.ecap = tp.ecap;
                            ta.rec = tp.rec;
                            t1_sort<false>(ta, tp.nbins, Mp, xyz, L.d_t2_meta, L.d_t2_binstart, L.d_t2_rec, P, ls);
                        }
                        for (const Pair &pr : pairs) {
                            if (pr.n == 0) continue;
                            const int64_t nu = pr.ustart ? pr.nu : pr.n, np = pr.adj_np;
                            if (!t2) {
                                const T *pos = pr.adj_pos->template as<T>();
                                // sources: the pair's distinct vectors; targets: the directions, scaled per channel
                                P.set_geometry(adj_c(pr), adj_B(pr), xc, X, smax);
                                P.set_sources(np, pos, pos + np, D > 2 ? pos + 2 * np : nullptr);
                            }
                            AdjStrengthArgs sa{};
                            sa.nu = nu;
                            sa.nfg = nfg;
                            sa.tpol = tpol;
                            sa.g_f_stride = (int64_t)nt * per_tf;
                            for (int r = 0; r < 4; ++r) sa.pol_off[r] = pol_off[r];
                            sa.transpose_flipped = !reference_compat;
                            cplx<T> *q = L.d_adj_q.template as<cplx<T>>();
                            if (nbasis) {
                                const AdjBasisArgs ba{pr.bi, pr.bj, nbasis, (int)freqs.size(), fa, np > nu ? 1 : 0};
                                hipLaunchKernelGGL(k_adj_strengths_basis<T>, dim3((unsigned)cdiv(nu * nfg * ADJ_GROUP, 256)), dim3(256), 0,
                                                   ls, sa, ba, dg + ((int64_t)(fa - f0) * nt + (t - t0)) * per_tf,
                                                   pr.trivial ? nullptr : pr.idx->template as<int>(),
                                                   pr.ustart ? pr.ustart->template as<int>() : nullptr,
                                                   d_coefs.as<cplx<T>>(), d_ant1.as<int>(), d_ant2.as<int>(), q, d_err.as<int>() + 4);
                            } else {
                                hipLaunchKernelGGL(k_adj_strengths<T>, dim3((unsigned)cdiv(nu * nfg * ADJ_GROUP, 256)), dim3(256), 0, ls, sa,
                                                   dg + ((int64_t)(fa - f0) * nt + (t - t0)) * per_tf,
                                                   pr.trivial ? nullptr : pr.idx->template as<int>(),
                                                   pr.trivial ? nullptr : pr.flip->template as<signed char>(),
                                                   pr.ustart ? pr.ustart->template as<int>() : nullptr, q, d_err.as<int>() + 4);
                            }
                            cplx<T> *zb = L.d_adj_z.template as<cplx<T>>();
                            if (t2) {
                                const int nplanes = nfg * tpol;
                                cplx<T> *A = P.fft_input(nplanes);
                                const int *cells = pr.t2_cells->template as<int>();
                                hipLaunchKernelGGL(k_t2_fill<T>, dim3((unsigned)cdiv((int64_t)g2.na * g2.na * nplanes, 256)), dim3(256), 0,
                                                   ls, g2.na, nplanes, nu, cells, cells + (size_t)g2.na * g2.na + 1, (const cplx<T> *)q,
                                                   (const T *)L.d_t2_dec.template as<T>(), A);
                                P.fft(nplanes);
                                // entries past the live count do not exist: their slots of z are never read
                                const int Tt = (1 << BINLOG) + ta.w - 1;
                                const size_t lds = sizeof(cplx<T>) * (size_t)tpol * Tt * Tt;
                                hipLaunchKernelGGL((polarized ? k_t2_gather<T, 4> : k_t2_gather<T, 1>), dim3((unsigned)(nfg * tp.nb1 * tp.nb1)),
                                                   dim3(T2_THREADS), lds, ls, ta, g2.P, g2.cnt(), (const unsigned char *)L.d_t2_rec.template as<unsigned char>(),
                                                   (const int *)L.d_t2_binstart.template as<int>(), P.fft_output(), zb);
                                st[ST_SPREAD_LAUNCHES] += 1;
                                st[ST_GATHERED] += (double)cap * nplanes;
                                st[ST_N2X] = st[ST_N2Y] = g2.n2;
                                st[ST_NA_XY] = g2.na * 65536.0 + g2.na;
                                st[ST_W] = ta.w;
                                st[ST_SIGMA] = sigma_a;
                            } else {
                                P.load_strengths(q, nfg * tpol, tpol, d_freqs.as<double>() + fa);
                                P.spread(nfg * tpol);
                                P.fft(nfg * tpol);
                                // every slot of the compacted arrays is a target (the live count stays on the device): slots
                                // past it are computed and never read
                                P.interp(cap, xyz, xyz + cap, D > 2 ? xyz + 2 * cap : nullptr, nullptr, nullptr,
                                         d_freqs.as<double>() + fa, nfg, tpol, zb, (int64_t)tpol * cap, 1, z_off, false);
                            }
                            AdjAccArgs aa{};
                            aa.M = cap;
                            aa.nfg = nfg;
                            aa.f_first = fa;
                            aa.f_base = fb.b0;
                            aa.nfa = nfa;
                            aa.polarized = polarized;
                            aa.pol_sky = pol_sky;
                            aa.same_beam = pr.bi == pr.bj;
                            aa.bi = desc(pr.bi);
                            aa.bj = desc(pr.bj);
                            hipLaunchKernelGGL((ord == 3 ? k_adj_accumulate<T, 3> : ord == 1 ? k_adj_accumulate<T, 1> : k_adj_accumulate<T, 0>),
                                               dim3((unsigned)cdiv(cap * nfg, 256)), dim3(256), 0, ls, aa, Mp,
                                               L.d_srcidx.template as<int>(), L.d_az.template as<T>(), L.d_za.template as<T>(),
                                               d_freqs.as<double>(), zb, L.d_adj_acc.template as<double>());
                        }
                    }
                }
            }
            for (int li = 1; li < nlanes; ++li) {  // join: the reduction on the main stream sees every lane
                FV_HIP(hipEventRecord(lanes[li].done, lanes[li].stream));
                FV_HIP(hipStreamWaitEvent(stream, lanes[li].done, 0));
            }
            AdjReduceArgs ra{};
            for (int li = 0; li < nlanes; ++li) ra.acc[li] = lanes[li].d_adj_acc.template as<double>();
            ra.nl = nlanes;
            ra.nfa = nfa;
            ra.f_base = fb.b0;
            ra.nfreq = nfreq_cat;
            ra.comps = comps;
            ra.nsrc = nsrc;
            const int64_t ne = nsrc * nfa * comps;
            if (ne > 0) hipLaunchKernelGGL(k_adj_reduce<T>, dim3((unsigned)cdiv(ne, 256)), dim3(256), 0, stream, ra, dgf);
        }
        if (!gflux_on_device && gf_bytes) FV_HIP(hipMemcpyAsync(gflux, dgf, gf_bytes, hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
    }

    void adjoint_release() {
        // The call ends synchronised.  Its own bulk device memory -- the second transforms' grids, their values at the
        // directions, the accumulators, the staged G and gflux -- is given back when it exceeds FFTVIS_HIP_ADJ_KEEP_BYTES
        // (default 256 MiB): a cached handle then holds for its next forward run what it held before, but for the adjoint
        // plans' tables and per-baseline arrays.  Smaller sets stay for the next call (freeing and reallocating them
        // doubled a C2 adjoint step).  The basis adjoint's inner products S and staged gcoefs count and go likewise, and so
        // do the type-2 path's planes and entry records.
        FV_HIP(hipStreamSynchronize(stream));
        {
            size_t bulk = d_adj_g.cap + d_adj_gf.cap + d_adj_gc.cap;
            for (Lane &L : lanes)
                bulk += L.d_adj_z.cap + L.d_adj_acc.cap + L.d_gs.cap + (L.adj ? L.adj->buf0.cap + L.adj->buf1.cap : 0) +
                        L.d_t2_rec.cap + L.d_t2_meta.cap + L.d_t2_binstart.cap + (L.adj2 ? L.adj2->buf0.cap + L.adj2->buf1.cap : 0);
            const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
            if ((double)bulk > (ek ? std::atof(ek) : 256.0 * 1024 * 1024)) {
                for (Lane &L : lanes) {
                    if (L.adj) {
                        L.adj->buf0.release();
                        L.adj->buf1.release();
                    }
                    if (L.adj2) {
                        L.adj2->buf0.release();
                        L.adj2->buf1.release();
                    }
                    L.d_t2_rec.release();
                    L.d_t2_meta.release();
                    L.d_t2_binstart.release();
                    L.d_adj_z.release();
                    L.d_adj_acc.release();
                    L.d_gs.release();
                }
                d_adj_g.release();
                d_adj_gf.release();
                d_adj_gc.release();
            }
        }
    }

    // ---- basis beams: gradients with respect to the fluxes (gflux += A^T G, as run_adjoint defines it) and to the
    // coefficients, Re <dV[C; D], G> = Re <D, gcoefs> for every complex direction D (DESIGN.md "Adjoint") ------------------
    // Flux pass: adjoint_flux.  Coefficient pass: the forward run's own stages with the gather's gradient epilogue
    // (k_interp<.., GRAD>), which reads G where the forward writes V and adds the inner products S_kl(b) to the fp64 S
    // buffer of its stream, across time steps, source chunks and height terms; k_coef_reduce then sums the buffers in lane
    // order and contracts with C.  S is (K^2, channels of a block, nbls) complex fp64: channel blocks keep one buffer under
    // FFTVIS_HIP_ADJ_ACC_BYTES (default 256 MiB), each block a forward run over its channels.
    void run_basis_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                           int gflux_on_device, void *gcoefs, int gcoefs_on_device, int accumulate) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nbasis > 0, "fv_sim_run_basis_adjoint needs a handle with basis beams (fv_sim_set_basis)");
        FV_REQUIRE(!type1, "basis beams never take the lattice path");
        check_run(t0, t1, f0, f1);
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        // a host G is staged once for both passes
        FV_HIP(hipStreamSynchronize(stream));
        const int64_t g_elems = (int64_t)nf * nt * per_tf;
        const cplx<T> *dg = (const cplx<T> *)gvis;
        if (!gvis_on_device) {
            upload(d_adj_g, gvis, sizeof(cplx<T>) * (size_t)g_elems, 0);
            dg = d_adj_g.as<cplx<T>>();
        }
        if (g_elems > 0) {  // NaN in G fails the call before either pass runs
            hipLaunchKernelGGL(k_count_nan<T>, dim3((unsigned)std::min<int64_t>(cdiv(g_elems, 256), 4096)), dim3(256), 0, stream, dg,
                               g_elems, d_err.as<int>() + 4);
            check_errors();
        }
        if (gflux) adjoint_flux(t0, t1, f0, f1, dg, 1, gflux, gflux_on_device, accumulate);
        if (gcoefs) coef_pass(t0, t1, f0, f1, dg, gcoefs, gcoefs_on_device, accumulate);
        adjoint_release();
        check_errors();
    }

    void coef_pass(int t0, int t1, int f0, int f1, const cplx<T> *dg, void *gcoefs, int gcoefs_on_device, int accumulate) {
        const int nt = t1 - t0, nf = f1 - f0, K = nbasis, nfreq = (int)freqs.size();
        const int64_t per_tf = (int64_t)tpol * nbls;
        // the adjoint's transforms (or an earlier run) may have the lanes busy, and its runs were built on three components
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        const size_t gc_bytes = sizeof(cplx<T>) * (size_t)nant_basis * K * nfreq;
        cplx<T> *dgc = (cplx<T> *)gcoefs;
        if (!gcoefs_on_device) {
            d_adj_gc.reserve(std::max<size_t>(gc_bytes, 16));
            dgc = d_adj_gc.as<cplx<T>>();
            if (accumulate) FV_HIP(hipMemcpyAsync(dgc, gcoefs, gc_bytes, hipMemcpyHostToDevice, stream));
        }
        if (!accumulate) FV_HIP(hipMemsetAsync(dgc, 0, gc_bytes, stream));
        const char *eab = std::getenv("FFTVIS_HIP_ADJ_ACC_BYTES");
        const double acc_max = eab ? std::atof(eab) : 256.0 * 1024 * 1024;
        const double per_chan = 16.0 * K * K * (double)std::max<int64_t>(nbls, 1);
        const int nfb = (int)std::max<double>(1.0, std::min<double>(nf, std::floor(acc_max / per_chan)));
        for (int b0 = f0; b0 < f1 && nt > 0; b0 += nfb) {
            const int b1 = std::min(f1, b0 + nfb), nfa = b1 - b0;
            if (mhist_log.size() > 65536) mhist_log.clear();
            RunPlan r{t0, t1, b0, b1, nt, nfa};
            source_box(r.xc, r.X);
            height_terms(r);
            pair_setup(r);
            grid_and_groups(r);
            light_classes(r);
            lane_schedule(r);
            lane_plans(r);
            r.ch = source_chunks(r.nlanes_used);
            lane_buffers(r);
            // one S buffer per stream that runs gathers: the main stream's when the lanes are pipelined, else one per lane
            const int ns = r.pipe ? 1 : r.nlanes;
            const size_t s_bytes = sizeof(cplx<double>) * (size_t)K * K * nfa * (size_t)std::max<int64_t>(nbls, 1);
            cplx<double> *gs[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int li = 0; li < ns; ++li) {
                lanes[li].d_gs.reserve(s_bytes);
                gs[li] = lanes[li].d_gs.template as<cplx<double>>();
                FV_HIP(hipMemsetAsync(gs[li], 0, s_bytes, stream));  // (the lanes start after what the main stream holds now)
            }
            OutBlock o{};
            o.out = nullptr;
            o.on_device = true;
            o.nt = nt;
            o.nf = nfa;
            o.dout = const_cast<cplx<T> *>(dg) + (int64_t)(b0 - f0) * nt * per_tf;  // read only: the gradient epilogue never writes it
            o.per_tf = per_tf;
            o.run = (int64_t)nt * per_tf;
            o.fs = o.run;
            o.bytes = sizeof(cplx<T>) * (size_t)nfa * o.run;
            o.run_bytes = sizeof(cplx<T>) * (size_t)o.run;
            o.shared = false;
            o.drain = false;
            Drain dr;
            queue_units(r, o, dr, gs);
            CoefReduceArgs ca{};
            for (int li = 0; li < ns; ++li) ca.S[li] = gs[li];
            ca.nl = ns;
            ca.K = K;
            ca.nfa = nfa;
            ca.f_base = b0;
            ca.nfreq = nfreq;
            ca.nant = nant_basis;
            ca.nbls = nbls;
            const int64_t items = (int64_t)nant_basis * K * nfa;
            hipLaunchKernelGGL(k_coef_reduce<T>, dim3((unsigned)cdiv(items, 4)), dim3(256), 0, stream, ca, d_csr_start.as<int>(),
                               d_csr.as<int>(), d_ant1.as<int>(), d_ant2.as<int>(), d_coefs.as<cplx<T>>(), dgc);
        }
        if (!gcoefs_on_device) FV_HIP(hipMemcpyAsync(gcoefs, dgc, gc_bytes, hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
    }

    // ---- positions: gbls += the gradient with respect to the baseline vectors (DESIGN.md "Adjoint") -------------------
    // Every forward path approximates out_k = cj_k( sum_j c_j exp(i nu s_k b'_k . x_j) ), b' = R b / c the array as set,
    // x = 2 pi R topo; the strengths do not depend on the positions, so d out_k / d b'_k,d = i nu D'_d with D'_d what the
    // forward writes when every source's strengths are multiplied by x_j,d (a flipped baseline conjugates -i nu X to
    // +i nu conj(X): no sign case remains).  With G = dL/dV, dL = Re sum conj(G) dV:
    //     g'[k, d] = - sum_{f, t, r} nu_f Im( conj(G) D'_d ),     gbls[k] = R^T g'[k] / c   (per metre, in the frame of b).
    // The pass is coef_pass's: per channel block the forward's own stages; per (time, chunk, group, pair, height term) one
    // k_strengths_moments launch and three rounds of spread -> FFT -> gradient gather (k_interp<.., GRAD> without basis
    // beams) into the (3, channels of the block, nbls) complex fp64 S buffer of the stream; k_posgrad_reduce contracts.
    // Basis beams (fv_sim_run_basis_position_adjoint): V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b) and every M_kl is such a
    // sum with strengths that do not depend on the positions, so D'_d is the basis forward of the strengths times x_d: the
    // same rounds per (k <= l) term (and per form of the (l, k) term, as in the forward), the gather applying the basis
    // weights (k_interp<.., BPOS = 1>) and every term adding into the SAME (3, channels, nbls) S -- it does not grow by K^2.
    void run_position_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gbls,
                              int gbls_on_device, int accumulate, bool basis) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(!type1, "the position adjoint runs the type-3 transform: set the array with fv_sim_set_array, not "
                           "fv_sim_set_array_type1 (a lattice form of the pass does not exist)");
        if (basis)
            FV_REQUIRE(nbasis > 0, "fv_sim_run_basis_position_adjoint needs a handle with basis beams (fv_sim_set_basis); "
                                   "without them fv_sim_run_position_adjoint is the pass");
        else
            FV_REQUIRE(nbasis == 0, "the position adjoint does not cover basis beams (fv_sim_set_basis / beam_coefs)");
        check_run(t0, t1, f0, f1);
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        // an earlier run may have the lanes busy
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        const int64_t g_elems = (int64_t)nf * nt * per_tf;
        const cplx<T> *dg = (const cplx<T> *)gvis;
        if (!gvis_on_device) {
            upload(d_adj_g, gvis, sizeof(cplx<T>) * (size_t)g_elems, 0);
            dg = d_adj_g.as<cplx<T>>();
        }
        if (g_elems > 0) {  // NaN in G fails the call before anything runs
            hipLaunchKernelGGL(k_count_nan<T>, dim3((unsigned)std::min<int64_t>(cdiv(g_elems, 256), 4096)), dim3(256), 0, stream, dg,
                               g_elems, d_err.as<int>() + 4);
            check_errors();
        }
        const size_t gb_bytes = sizeof(double) * 3 * (size_t)nbls;
        double *dgb = gbls;
        if (!gbls_on_device) {
            d_adj_gf.reserve(std::max<size_t>(gb_bytes, 16));
            dgb = d_adj_gf.as<double>();
            if (accumulate) FV_HIP(hipMemcpyAsync(dgb, gbls, gb_bytes, hipMemcpyHostToDevice, stream));
        }
        if (!accumulate) FV_HIP(hipMemsetAsync(dgb, 0, gb_bytes, stream));
        const char *eab = std::getenv("FFTVIS_HIP_ADJ_ACC_BYTES");
        const double acc_max = eab ? std::atof(eab) : 256.0 * 1024 * 1024;
        const double per_chan = 16.0 * 3 * (double)std::max<int64_t>(nbls, 1);
        const int nfb = (int)std::max<double>(1.0, std::min<double>(nf, std::floor(acc_max / per_chan)));
        for (int b0 = f0; b0 < f1 && nt > 0 && nbls > 0; b0 += nfb) {
            const int b1 = std::min(f1, b0 + nfb), nfa = b1 - b0;
            if (mhist_log.size() > 65536) mhist_log.clear();
            RunPlan r{t0, t1, b0, b1, nt, nfa};
            r.moments = true;
            source_box(r.xc, r.X);
            height_terms(r);
            pair_setup(r);
            grid_and_groups(r);
            light_classes(r);
            lane_schedule(r);
            lane_plans(r);
            r.ch = source_chunks(r.nlanes_used);
            lane_buffers(r);
            // one S buffer per stream that runs gathers: the main stream's when the lanes are pipelined, else one per lane
            const int ns = r.pipe ? 1 : r.nlanes;
            const size_t s_bytes = sizeof(cplx<double>) * 3 * (size_t)nfa * (size_t)nbls;
            cplx<double> *gs[4] = {nullptr, nullptr, nullptr, nullptr};
            for (int li = 0; li < ns; ++li) {
                lanes[li].d_gs.reserve(s_bytes);
                gs[li] = lanes[li].d_gs.template as<cplx<double>>();
                FV_HIP(hipMemsetAsync(gs[li], 0, s_bytes, stream));  // (the lanes start after what the main stream holds now)
            }
            OutBlock o{};
            o.out = nullptr;
            o.on_device = true;
            o.nt = nt;
            o.nf = nfa;
            o.dout = const_cast<cplx<T> *>(dg) + (int64_t)(b0 - f0) * nt * per_tf;  // read only: the gradient epilogue never writes it
            o.per_tf = per_tf;
            o.run = (int64_t)nt * per_tf;
            o.fs = o.run;
            o.bytes = sizeof(cplx<T>) * (size_t)nfa * o.run;
            o.run_bytes = sizeof(cplx<T>) * (size_t)o.run;
            o.shared = false;
            o.drain = false;
            Drain dr;
            queue_units(r, o, dr, gs);
            PosReduceArgs pa{};
            for (int li = 0; li < ns; ++li) pa.S[li] = gs[li];
            pa.nl = ns;
            pa.nfa = nfa;
            pa.f_base = b0;
            pa.nbls = nbls;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) pa.rt[3 * i + j] = rplane.m[3 * j + i] / SPEED_OF_LIGHT;
            hipLaunchKernelGGL(k_posgrad_reduce, dim3((unsigned)cdiv(nbls * POS_GROUP, 256)), dim3(256), 0, stream, pa,
                               d_freqs.as<double>(), dgb);
        }
        if (!gbls_on_device) FV_HIP(hipMemcpyAsync(gbls, dgb, gb_bytes, hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
        // the three strength sets belong to this pass: beyond the keep limit the lanes' strength buffers go back too (the
        // next run's lane_buffers sizes them again before it queues anything)
        {
            size_t str = 0;
            for (Lane &L : lanes)
                for (auto &P : L.plan)
                    if (P) str += P->strengths.cap;
            const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
            if ((double)str > (ek ? std::atof(ek) : 256.0 * 1024 * 1024))
                for (Lane &L : lanes)
                    for (auto &P : L.plan)
                        if (P) P->strengths.release();
        }
        adjoint_release();
        check_errors();
    }

    // ---- sources: gtopo[t - t0] += the tangential gradient with respect to the sources' ENU unit vectors at time t ------
    // (DESIGN.md "Sources"; the kernels' comment above k_src_moments).  adjoint_flux's set-up and loop -- channel blocks,
    // lanes, source chunks, horizon_step, k_adj_strengths and the type-3 transform with the roles swapped -- with 1 + D
    // rounds of load -> spread -> FFT -> interp per (time, chunk, group, pair): the strengths q, then q times each
    // coordinate of the run's vector (k_src_moments; D = 2 on coplanar handles, where Z does not depend on the third
    // coordinate).  k_src_accumulate contracts with the forward's strengths and adds the beam term; the accumulator is
    // per time step, and k_srcgrad_reduce writes the step's rows on the lane's own stream.
    // Basis beams (fv_sim_run_basis_source_adjoint): V_b = sum_kl (w1 M_kl(b), w2 M_kl(b) or conj(M_kl(-b))^T) and every
    // M_kl is such a sum with the strengths c^{kl} of basis beams k and l, so the pairs are the (k <= l) terms as in
    // adjoint_flux's basis mode: k_adj_strengths_basis writes the term's weighted q -- in the exact form the mirrored half
    // at -b follows the plain one, and the moments take its coordinates -b like any other source's --, the 1 + D rounds
    // run over nu or 2 nu sources, and k_src_accumulate contracts with the term's beams.  Every term adds into the lane's
    // accumulator in stream order; the reduction runs once per time step, after the last term.
    //
    // Joint pass (fv_sim_run_sky_adjoint, fv_sim_run_basis_sky_adjoint: gflux given): set 0 of the 1 + D rounds is the Z
    // adjoint_flux computes -- the same strengths, plan parameters and targets --, so k_adj_accumulate contracts it with the
    // pair's or term's beams at the lane's az / za into a flux accumulator of the lane's own, which follows the lane's 3
    // doubles per (source, channel) in d_adj_acc and lives for a channel block; k_adj_reduce then sums the lanes in lane
    // order into gflux on the main stream, as in adjoint_flux.  Without gflux nothing here differs from the pass above.
    void run_source_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gtopo,
                            int gtopo_on_device, int accumulate, bool basis) override {
        source_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, nullptr, 0, gtopo, gtopo_on_device, accumulate, basis);
    }
    void run_sky_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux, int gflux_on_device,
                         double *gtopo, int gtopo_on_device, int accumulate, bool basis) override {
        FV_REQUIRE(gflux, "null flux gradient");
        source_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, gtopo, gtopo_on_device, accumulate, basis);
    }
    void source_adjoint(int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux, int gflux_on_device,
                        double *gtopo, int gtopo_on_device, int accumulate, bool basis) {
        FV_HIP(hipSetDevice(device));
        if (gflux) {
            FV_REQUIRE(!type1, "the sky adjoint runs the type-3 transform: set the array with fv_sim_set_array, not "
                               "fv_sim_set_array_type1");
            if (basis)
                FV_REQUIRE(nbasis > 0, "fv_sim_run_basis_sky_adjoint needs a handle with basis beams (fv_sim_set_basis); "
                                       "without them fv_sim_run_sky_adjoint is the pass");
            else
                FV_REQUIRE(nbasis == 0, "the sky adjoint does not cover basis beams (fv_sim_set_basis / beam_coefs): "
                                        "fv_sim_run_basis_sky_adjoint does");
        } else {
            FV_REQUIRE(!type1, "the source adjoint runs the type-3 transform: set the array with fv_sim_set_array, not "
                               "fv_sim_set_array_type1");
            if (basis)
                FV_REQUIRE(nbasis > 0, "fv_sim_run_basis_source_adjoint needs a handle with basis beams (fv_sim_set_basis); "
                                       "without them fv_sim_run_source_adjoint is the pass");
            else
                FV_REQUIRE(nbasis == 0, "the source adjoint does not cover basis beams (fv_sim_set_basis / beam_coefs)");
        }
        check_run(t0, t1, f0, f1);
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        if (copy_stream) FV_HIP(hipStreamSynchronize(copy_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        for (Lane &L : lanes) {
            L.heavy_pending = false;
            for (int &b : L.binned_ti) b = -1;
        }
        lane_mode = -1;
        const double tol = dedup_tol();
        for (Pair &p : pairs) build_unique(p, tol, 3);
        const int D = dim(), nsets = 1 + D;
        double xc[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
        source_box(xc, X);
        // the NUFFT sources of every pair are adjoint_flux's (adj_sources): in the exact basis form an off-diagonal term's
        // mirrored set follows the plain one, in a box symmetric about 0
        auto adj_c = [&](const Pair &p) { return adj_mirrored(p) ? (const double *)zero3 : (const double *)p.btc; };
        auto adj_B = [&](const Pair &p) { return adj_mirrored(p) ? (const double *)p.Bs : (const double *)p.B; };
        adj_sources(D);
        const int64_t g_elems = (int64_t)nf * nt * per_tf;
        const cplx<T> *dg = (const cplx<T> *)gvis;
        if (!gvis_on_device) {
            upload(d_adj_g, gvis, sizeof(cplx<T>) * (size_t)g_elems, 0);
            dg = d_adj_g.as<cplx<T>>();
        }
        if (g_elems > 0) {  // NaN in G fails the call before anything runs
            hipLaunchKernelGGL(k_count_nan<T>, dim3((unsigned)std::min<int64_t>(cdiv(g_elems, 256), 4096)), dim3(256), 0, stream, dg,
                               g_elems, d_err.as<int>() + 4);
            check_errors();
        }
        int64_t nu_max = 1;
        for (const Pair &p : pairs) nu_max = std::max<int64_t>(nu_max, p.n ? p.adj_np : 0);
        const double cells2 = cells_at_sigma2(X, D, f0, f1, adj_B);
        const double sigma_a = this->sigma != 0.0 ? this->sigma : auto_sigma(cells2, 0.5 * (double)nsrc + (double)nu_max, D);
        const double cells_top = 2.0 * cells2 * (sigma_a == 2.0 ? 1.0 : std::pow(1.25 / 2.0, D));
        const char *el = std::getenv("FFTVIS_HIP_LANES");
        const int nlanes = std::max(1, std::min(2, std::min(el ? std::atoi(el) : 2, std::max(nt, 1))));
        const Chunks sc = source_chunks(nlanes);
        const int nch = sc.n;
        const int64_t csz = sc.csz, cap = sc.cap;
        // channel blocks: a lane's accumulator holds nsrc x (channels of a block) x 3 doubles, at most
        // FFTVIS_HIP_ADJ_ACC_BYTES; every block walks the time steps once.  Joint pass: comps more for the fluxes
        const int comps = pol_sky ? 8 : 1;
        const double acc_per = gflux ? 24.0 + 8.0 * comps : 24.0;
        const char *eab = std::getenv("FFTVIS_HIP_ADJ_ACC_BYTES");
        const double acc_max = eab ? std::atof(eab) : 256.0 * 1024 * 1024;
        const int nfb = (int)std::max<double>(1.0, std::min<double>(nf, std::floor(acc_max / (acc_per * std::max<int64_t>(nsrc, 1)))));
        struct FBlock {
            int b0, b1;
            std::vector<std::pair<int, int>> groups;
        };
        std::vector<FBlock> fblocks;
        int nfg_max = 1;
        for (int b0 = f0; b0 < f1; b0 += nfb) {
            FBlock fb{b0, std::min(f1, b0 + nfb), {}};
            fb.groups = freq_groups(fb.b0, fb.b1, cells_top, tpol);
            for (const auto &grp : fb.groups) nfg_max = std::max(nfg_max, grp.second - grp.first);
            fblocks.push_back(std::move(fb));
        }
        // the flux accumulator (joint pass) starts facc_off doubles into the lane's d_adj_acc
        const size_t facc_off = 3 * (size_t)std::max<int64_t>(nsrc * std::min(nf, nfb), 1);
        const size_t acc_bytes =
            sizeof(double) * (facc_off + (gflux ? (size_t)std::max<int64_t>(nsrc * std::min(nf, nfb) * comps, 1) : 0));
        for (int li = 0; li < nlanes; ++li) {
            Lane &L = lanes[li];
            if (!L.adj || L.adj->dim != D || L.adj->sigma != sigma_a || L.adj->eps != eps)
                L.adj.reset(new Nufft3<T>(D, eps, sigma_a, L.stream));
            L.adj->stream = L.stream;
            L.adj->err_oob = d_err.as<int>();
            L.adj->disc_radius = 0.0;  // its sources are baselines
            L.adj->transpose_flipped = false;
            L.adj->arm_columns(nullptr, nullptr, tpol, 0);
            // 1 + D sets of strengths and of values at the directions: the extra capacity belongs to this pass
            L.d_adj_q.reserve(sizeof(cplx<T>) * (size_t)nu_max * nfg_max * tpol * nsets);
            L.d_adj_z.reserve(sizeof(cplx<T>) * (size_t)cap * nfg_max * tpol * nsets);
            L.d_adj_acc.reserve(acc_bytes);
        }
        const size_t gt_bytes = sizeof(double) * 3 * (size_t)nsrc * (size_t)nt;
        double *dgt = gtopo;
        // joint pass: gflux on the device as in adjoint_flux; a host gflux is staged behind a host gtopo in d_adj_gf
        const size_t gf_bytes = gflux ? sizeof(T) * (size_t)nsrc * nfreq_cat * comps : 0;
        const size_t gt_stage = gtopo_on_device ? 0 : std::max<size_t>(gt_bytes, 16);
        const size_t gf_stage = gflux && !gflux_on_device ? std::max<size_t>(gf_bytes, 16) : 0;
        const size_t gf_at = (gt_stage + 255) / 256 * 256;
        T *dgf = (T *)gflux;
        if (gt_stage + gf_stage) d_adj_gf.reserve(gf_stage ? gf_at + gf_stage : gt_stage);
        if (!gtopo_on_device) {
            dgt = d_adj_gf.as<double>();
            if (accumulate && gt_bytes) FV_HIP(hipMemcpyAsync(dgt, gtopo, gt_bytes, hipMemcpyHostToDevice, stream));
        }
        if (!accumulate && gt_bytes) FV_HIP(hipMemsetAsync(dgt, 0, gt_bytes, stream));
        if (gflux && !gflux_on_device) {
            dgf = (T *)((char *)d_adj_gf.p + gf_at);
            if (accumulate && gf_bytes) FV_HIP(hipMemcpyAsync(dgf, gflux, gf_bytes, hipMemcpyHostToDevice, stream));
        }
        if (gflux && !accumulate && gf_bytes) FV_HIP(hipMemsetAsync(dgf, 0, gf_bytes, stream));
        // the lanes write gtopo's rows themselves: they start after the main stream has prepared it
        FV_HIP(hipEventRecord(ev_start, stream));
        for (int li = 0; li < nlanes; ++li)
            if (lanes[li].stream != stream) FV_HIP(hipStreamWaitEvent(lanes[li].stream, ev_start, 0));
        const std::array<int64_t, 16> pol_off = pol_offsets();  // the forward's output slots
        int64_t z_off[16] = {0};
        for (int r = 0; r < tpol; ++r) z_off[r] = (int64_t)r * cap;
        const int ord = beam_order == 3 ? 3 : beam_order == 1 ? 1 : 0;
        for (size_t bi = 0; bi < fblocks.size(); ++bi) {
            const FBlock &fb = fblocks[bi];
            const int nfa = fb.b1 - fb.b0;
            for (int li = 0; gflux && li < nlanes; ++li) {  // the lanes' flux accumulators, as adjoint_flux starts a block
                if (bi > 0 && lanes[li].stream != stream) {  // the previous block's reduction has read this accumulator
                    FV_HIP(hipEventRecord(ev_start, stream));
                    FV_HIP(hipStreamWaitEvent(lanes[li].stream, ev_start, 0));
                }
                FV_HIP(hipMemsetAsync(lanes[li].d_adj_acc.template as<double>() + facc_off, 0,
                                      sizeof(double) * (size_t)std::max<int64_t>(nsrc * nfa * comps, 1), lanes[li].stream));
            }
            for (int t = t0; t < t1 && nsrc > 0; ++t) {
                Lane &L = lanes[(t - t0) % nlanes];
                const hipStream_t ls = L.stream;
                Nufft3<T> &P = *L.adj;
                double *acc = L.d_adj_acc.template as<double>();
                FV_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 3 * (size_t)nsrc * nfa, ls));
                const T *vec = nullptr;
                for (int ch = 0; ch < nch; ++ch) {
                    const int64_t s0 = (int64_t)ch * csz, sn = std::min<int64_t>(csz, nsrc - s0);
                    if (sn <= 0) continue;
                    const int *Mp = horizon_step(L, t, cap, sc.nblk, ls, s0, sn, (int64_t)t * nch + ch);
                    // the vectors horizon_step read (every chunk of a time step writes its own range of the lane's d_enu)
                    vec = !astroms.empty() ? L.d_enu.template as<T>()
                                           : ntimes_topo ? d_topo.as<T>() + (size_t)t * 3 * nsrc : d_eq.as<T>();
                    const T *xyz = L.d_xyz.template as<T>();
                    for (const auto &grp : fb.groups) {
                        const int fa = grp.first, nfg = grp.second - grp.first;
                        const double smax = fmax_of(fa, grp.second);
                        const int ntr = nfg * tpol;
                        for (const Pair &pr : pairs) {
                            if (pr.n == 0) continue;
                            const int64_t nu = pr.adj_np;                        // sources of the transform
                            const int64_t nr = pr.ustart ? pr.nu : pr.n;         // runs of the list (nu / 2 with a mirrored set)
                            const T *pos = pr.adj_pos->template as<T>();
                            P.set_geometry(adj_c(pr), adj_B(pr), xc, X, smax);
                            P.set_sources(nu, pos, pos + nu, D > 2 ? pos + 2 * nu : nullptr);
                            AdjStrengthArgs sa{};
                            sa.nu = nr;
                            sa.nfg = nfg;
                            sa.tpol = tpol;
                            sa.g_f_stride = (int64_t)nt * per_tf;
                            for (int r = 0; r < 4; ++r) sa.pol_off[r] = pol_off[r];
                            sa.transpose_flipped = !reference_compat;
                            cplx<T> *q = L.d_adj_q.template as<cplx<T>>();
                            if (nbasis) {
                                const AdjBasisArgs ba{pr.bi, pr.bj, nbasis, (int)freqs.size(), fa, nu > nr ? 1 : 0};
                                hipLaunchKernelGGL(k_adj_strengths_basis<T>, dim3((unsigned)cdiv(nr * nfg * ADJ_GROUP, 256)), dim3(256), 0,
                                                   ls, sa, ba, dg + ((int64_t)(fa - f0) * nt + (t - t0)) * per_tf,
                                                   pr.trivial ? nullptr : pr.idx->template as<int>(),
                                                   pr.ustart ? pr.ustart->template as<int>() : nullptr,
                                                   d_coefs.as<cplx<T>>(), d_ant1.as<int>(), d_ant2.as<int>(), q, d_err.as<int>() + 4);
                            } else {
                                hipLaunchKernelGGL(k_adj_strengths<T>, dim3((unsigned)cdiv(nr * nfg * ADJ_GROUP, 256)), dim3(256), 0, ls, sa,
                                                   dg + ((int64_t)(fa - f0) * nt + (t - t0)) * per_tf,
                                                   pr.trivial ? nullptr : pr.idx->template as<int>(),
                                                   pr.trivial ? nullptr : pr.flip->template as<signed char>(),
                                                   pr.ustart ? pr.ustart->template as<int>() : nullptr, q, d_err.as<int>() + 4);
                            }
                            const int64_t q_set = nu * ntr, z_set = cap * ntr;
                            hipLaunchKernelGGL(k_src_moments<T>, dim3((unsigned)cdiv(q_set, 256)), dim3(256), 0, ls, nu, (int64_t)ntr, D,
                                               pos, q, q_set);
                            cplx<T> *zb = L.d_adj_z.template as<cplx<T>>();
                            for (int s = 0; s < nsets; ++s) {
                                P.load_strengths(q + s * q_set, ntr, tpol, d_freqs.as<double>() + fa);
                                P.spread(ntr);
                                P.fft(ntr);
                                // every slot of the compacted arrays is a target: slots past the live count are never read
                                P.interp(cap, xyz, xyz + cap, D > 2 ? xyz + 2 * cap : nullptr, nullptr, nullptr,
                                         d_freqs.as<double>() + fa, nfg, tpol, zb + s * z_set, (int64_t)tpol * cap, 1, z_off, false);
                            }
                            SrcAccArgs aa{};
                            aa.M = cap;
                            aa.nfg = nfg;
                            aa.f_first = fa;
                            aa.f_base = fb.b0;
                            aa.nfa = nfa;
                            aa.nfreq = nfreq_cat;
                            aa.polarized = polarized;
                            aa.pol_sky = pol_sky;
                            aa.same_beam = pr.bi == pr.bj;
                            aa.D = D;
                            aa.set_stride = z_set;
                            aa.vstride = nsrc;
                            aa.bi = desc(pr.bi);
                            aa.bj = desc(pr.bj);
                            aa.rt = rots[t];
                            aa.rp = rplane;
                            aa.h = sizeof(T) == 8 ? SRC_BEAM_STEP_FP64 : SRC_BEAM_STEP_FP32;
                            if (const char *eh = std::getenv("FFTVIS_HIP_SRC_BEAM_STEP")) aa.h = std::atof(eh);  // (measurements)
                            FV_REQUIRE(aa.h > 0.0 && aa.h < 1e-2, "FFTVIS_HIP_SRC_BEAM_STEP out of range");
                            hipLaunchKernelGGL((ord == 3 ? k_src_accumulate<T, 3> : ord == 1 ? k_src_accumulate<T, 1> : k_src_accumulate<T, 0>),
                                               dim3((unsigned)cdiv(cap * nfg, 256)), dim3(256), 0, ls, aa, Mp,
                                               L.d_srcidx.template as<int>(), vec, d_flux.p, d_freqs.as<double>(),
                                               (const cplx<T> *)zb, acc);
                            if (gflux) {  // set 0 is Z in k_adj_accumulate's layout: adjoint_flux's contraction
                                AdjAccArgs fx{};
                                fx.M = cap;
                                fx.nfg = nfg;
                                fx.f_first = fa;
                                fx.f_base = fb.b0;
                                fx.nfa = nfa;
                                fx.polarized = polarized;
                                fx.pol_sky = pol_sky;
                                fx.same_beam = pr.bi == pr.bj;
                                fx.bi = desc(pr.bi);
                                fx.bj = desc(pr.bj);
                                hipLaunchKernelGGL((ord == 3 ? k_adj_accumulate<T, 3> : ord == 1 ? k_adj_accumulate<T, 1> : k_adj_accumulate<T, 0>),
                                                   dim3((unsigned)cdiv(cap * nfg, 256)), dim3(256), 0, ls, fx, Mp,
                                                   L.d_srcidx.template as<int>(), L.d_az.template as<T>(), L.d_za.template as<T>(),
                                                   d_freqs.as<double>(), zb, acc + facc_off);
                            }
                        }
                    }
                }
                if (vec) {
                    SrcReduceArgs ra{};
                    ra.nsrc = nsrc;
                    ra.nfa = nfa;
                    ra.f_base = fb.b0;
                    ra.rt = rots[t];
                    ra.rp = rplane;
                    hipLaunchKernelGGL(k_srcgrad_reduce<T>, dim3((unsigned)cdiv(nsrc, 256)), dim3(256), 0, ls, ra, (const double *)acc, vec,
                                       d_freqs.as<double>(), dgt + (size_t)(t - t0) * 3 * nsrc);
                }
            }
            if (gflux) {  // the block's flux gradient: the lanes joined and summed in lane order on the main stream
                for (int li = 0; li < nlanes; ++li)
                    if (lanes[li].stream != stream) {
                        FV_HIP(hipEventRecord(lanes[li].done, lanes[li].stream));
                        FV_HIP(hipStreamWaitEvent(stream, lanes[li].done, 0));
                    }
                AdjReduceArgs ra{};
                for (int li = 0; li < nlanes; ++li) ra.acc[li] = lanes[li].d_adj_acc.template as<double>() + facc_off;
                ra.nl = nlanes;
                ra.nfa = nfa;
                ra.f_base = fb.b0;
                ra.nfreq = nfreq_cat;
                ra.comps = comps;
                ra.nsrc = nsrc;
                const int64_t ne = nsrc * nfa * comps;
                if (ne > 0) hipLaunchKernelGGL(k_adj_reduce<T>, dim3((unsigned)cdiv(ne, 256)), dim3(256), 0, stream, ra, dgf);
            }
        }
        for (int li = 0; li < nlanes; ++li)  // join: the copy on the main stream sees every lane
            if (lanes[li].stream != stream) {
                FV_HIP(hipEventRecord(lanes[li].done, lanes[li].stream));
                FV_HIP(hipStreamWaitEvent(stream, lanes[li].done, 0));
            }
        if (!gtopo_on_device && gt_bytes) FV_HIP(hipMemcpyAsync(gtopo, dgt, gt_bytes, hipMemcpyDeviceToHost, stream));
        if (gf_stage && gf_bytes) FV_HIP(hipMemcpyAsync(gflux, dgf, gf_bytes, hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
        {  // the 1 + D strength sets belong to this pass: beyond the keep limit they go back with the rest
            const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
            size_t qb = 0;
            for (Lane &L : lanes) qb += L.d_adj_q.cap + L.d_adj_z.cap;
            if ((double)qb > (ek ? std::atof(ek) : 256.0 * 1024 * 1024))
                for (Lane &L : lanes) L.d_adj_q.release();
        }
        adjoint_release();
        check_errors();
    }

    // ---- tangent: out = dV, the change of the visibilities along (dbls, dtopo) (DESIGN.md "Tangents") --------------------
    //     dV = sum_k dV/db_k . dbls[k]  +  sum_{t, j} dV/dn_j(t) . P_n dtopo[t - t0, j]
    // Both position derivatives of the exact map are forward transforms of other strengths: with b' = R b / c, x = 2 pi R n,
    //     baselines:  i nu (R dbls[k] / c)_d D'_d[k],             D'_d the forward of the strengths times x_d (k_strengths_moments),
    //     sources:    forward of dc  +  i nu b'_k,d X_d[k],       X_d the forward of the strengths times dx_d (k_strengths_tangent),
    // and a flipped baseline needs no sign case.  The pass is run_position_adjoint's: per channel block the forward's own
    // stages; per (time, chunk, group, pair, height term) one strengths launch per input and 3 and / or 1 + D rounds of
    // spread -> FFT -> tangent gather (k_interp<.., TANGENT>) ADDING into the zeroed output block.  A time step's slots are
    // written by its own lane's stream only, in order: no sum over lanes, bitwise reproducible for a lane count.  A host
    // destination receives the block in one copy at the end.
    // Basis beams (fv_sim_run_basis_position_tangent: dbls; fv_sim_run_basis_source_tangent: dtopo; one of them per call):
    // the rounds per (k <= l) term as in run_position_adjoint, k_strengths_tangent with the term's beams, a weighted
    // round's gather adding i nu w (w1 V, w2 V) with the basis weights (k_interp<.., BPOS = 2>) and the beam term's
    // round adding (w1 V, w2 V) as they are -- which is the forward's own basis gather on the set dc.
    void run_tangent(int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device, const double *dtopo,
                     int dtopo_on_device, void *out, int out_on_device, bool basis) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(!type1, "the tangent runs the type-3 transform: set the array with fv_sim_set_array, not "
                           "fv_sim_set_array_type1 (a lattice form of the pass does not exist)");
        if (basis) {
            FV_REQUIRE(nbasis > 0, "the tangents through basis beams (fv_sim_run_basis_position_tangent, "
                                   "fv_sim_run_basis_source_tangent) need a handle with basis beams (fv_sim_set_basis); "
                                   "without them fv_sim_run_tangent is the pass");
            FV_REQUIRE(!(dbls && dtopo), "the tangents through basis beams take baseline directions or source directions, "
                                         "one per call (no entry point passes both)");
        } else {
            FV_REQUIRE(nbasis == 0, "the tangent does not cover basis beams (fv_sim_set_basis / beam_coefs)");
        }
        FV_REQUIRE(dbls || dtopo, "neither tangent input is given (dbls and dtopo are both null)");
        check_run(t0, t1, f0, f1);
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        // an earlier run may have the lanes busy
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        if (copy_stream) FV_HIP(hipStreamSynchronize(copy_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        // the weights: rows 0-2 R dbls / c (seconds, the transforms' frame), rows 3-5 the baselines' own vectors
        std::vector<double> w((size_t)6 * std::max<int64_t>(nbls, 1), 0.0);
        if (dbls && nbls > 0) {
            std::vector<double> hb((size_t)3 * nbls);
            if (dbls_on_device)
                FV_HIP(hipMemcpy(hb.data(), dbls, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
            else
                std::memcpy(hb.data(), dbls, sizeof(double) * hb.size());
            for (double v : hb) FV_REQUIRE(std::isfinite(v), "dbls holds a value that is not finite");
            for (int64_t k = 0; k < nbls; ++k)
                for (int d = 0; d < 3; ++d)
                    w[(size_t)d * nbls + k] = (rplane.m[3 * d] * hb[3 * k] + rplane.m[3 * d + 1] * hb[3 * k + 1] +
                                               rplane.m[3 * d + 2] * hb[3 * k + 2]) / SPEED_OF_LIGHT;
        }
        for (int64_t i = 0; i < 3 * nbls; ++i) w[(size_t)3 * nbls + i] = h_bls[i];
        upload(d_tan_w, w.data(), sizeof(double) * w.size(), 0);
        const double *ddt = nullptr;
        const int64_t dt_elems = (int64_t)nt * nsrc * 3;
        if (dtopo) {
            ddt = dtopo;
            if (!dtopo_on_device) {
                upload(d_tan_dt, dtopo, sizeof(double) * (size_t)dt_elems, 0);
                ddt = d_tan_dt.as<double>();
            }
            if (dt_elems > 0) {  // a value that is not finite fails the call before anything runs
                hipLaunchKernelGGL(k_count_nonfinite, dim3((unsigned)std::min<int64_t>(cdiv(dt_elems, 256), 4096)), dim3(256), 0, stream,
                                   ddt, dt_elems, d_err.as<int>() + 4);
                int bad = 0;
                FV_HIP(hipMemcpyAsync(&bad, d_err.as<int>() + 4, sizeof(int), hipMemcpyDeviceToHost, stream));
                FV_HIP(hipStreamSynchronize(stream));
                if (bad) {
                    FV_HIP(hipMemsetAsync(d_err.as<int>() + 4, 0, sizeof(int), stream));
                    FV_HIP(hipStreamSynchronize(stream));
                    throw Error(FV_ERR_ARG, std::to_string(bad) + " entries of dtopo are not finite");
                }
            }
        }
        OutBlock o = out_block(nt, nf, out, out_on_device);  // on the device, zeroed
        o.drain = false;
        const char *eab = std::getenv("FFTVIS_HIP_ADJ_ACC_BYTES");  // channel blocks as the position pass cuts them
        const double acc_max = eab ? std::atof(eab) : 256.0 * 1024 * 1024;
        const double per_chan = 16.0 * 3 * (double)std::max<int64_t>(nbls, 1);
        const int nfb = (int)std::max<double>(1.0, std::min<double>(nf, std::floor(acc_max / per_chan)));
        for (int b0 = f0; b0 < f1 && nt > 0 && nbls > 0; b0 += nfb) {
            const int b1 = std::min(f1, b0 + nfb), nfa = b1 - b0;
            if (mhist_log.size() > 65536) mhist_log.clear();
            RunPlan r{t0, t1, b0, b1, nt, nfa};
            r.moments = dbls != nullptr;
            r.tan_w = d_tan_w.as<double>();
            if (ddt) {
                r.tan_dtopo = ddt;
                r.tan_D = dim();
                r.tan_sets = 1 + r.tan_D;
                r.tan_h = sizeof(T) == 8 ? SRC_BEAM_STEP_FP64 : SRC_BEAM_STEP_FP32;
                if (const char *eh = std::getenv("FFTVIS_HIP_SRC_BEAM_STEP")) r.tan_h = std::atof(eh);  // (measurements)
                FV_REQUIRE(r.tan_h > 0.0 && r.tan_h < 1e-2, "FFTVIS_HIP_SRC_BEAM_STEP out of range");
            }
            source_box(r.xc, r.X);
            height_terms(r);
            pair_setup(r);
            grid_and_groups(r);
            light_classes(r);
            lane_schedule(r);
            lane_plans(r);
            r.ch = source_chunks(r.nlanes_used);
            lane_buffers(r);
            OutBlock ob = o;  // this block's channels of the output
            ob.nf = nfa;
            ob.dout = o.dout + (int64_t)(b0 - f0) * nt * per_tf;
            ob.bytes = sizeof(cplx<T>) * (size_t)nfa * o.run;
            Drain dr;
            queue_units(r, ob, dr);
        }
        if (!o.on_device) copy_block_to_host(o, false, stream);
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
        // the strength sets and the staged inputs belong to this pass: beyond the keep limit they go back (the next run's
        // lane_buffers sizes the strength buffers again before it queues anything)
        {
            size_t str = d_tan_dt.cap + d_tan_w.cap;
            for (Lane &L : lanes)
                for (auto &P : L.plan)
                    if (P) str += P->strengths.cap;
            const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
            if ((double)str > (ek ? std::atof(ek) : 256.0 * 1024 * 1024)) {
                for (Lane &L : lanes)
                    for (auto &P : L.plan)
                        if (P) P->strengths.release();
                d_tan_dt.release();
                d_tan_w.release();
            }
        }
        adjoint_release();
        check_errors();
    }

    // ---- basis beams, forward mode: out[q] = dV[C; D_q], the change of the visibilities along the direction D_q of the
    // coefficients (DESIGN.md "Tangents") ----------------------------------------------------------------------------------
    // With V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b),
    //     dV_b[C; D] = sum_kl ( conj(D[a1,k]) C[a2,l] + conj(C[a1,k]) D[a2,l] ) M_kl(b),
    // and the basis visibilities M_kl depend on neither C nor D: the pass is ONE forward run -- its own stages over the
    // (k <= l) terms, packings, mirror gathers, height terms, column plans, lanes and source chunks -- whose gathers carry
    // the basis tangent epilogue (k_interp<.., BTAN>) and add every direction's weights times V into that direction's copy
    // of the zeroed output block.  The directions share every transform.  A time step's slots are written by its own lane's
    // stream only, in order: bitwise reproducible for a lane count.  A host destination receives the (ndir, ...) output in
    // one copy at the end.
    void run_basis_tangent(int t0, int t1, int f0, int f1, const void *dcoefs, int dcoefs_on_device, int ndir, void *out,
                           int out_on_device) override {
        FV_HIP(hipSetDevice(device));
        FV_REQUIRE(nbasis > 0, "fv_sim_run_basis_tangent needs a handle with basis beams (fv_sim_set_basis)");
        FV_REQUIRE(!type1, "basis beams never take the lattice path");
        check_run(t0, t1, f0, f1);
        const int nt = t1 - t0, nf = f1 - f0;
        const int64_t per_tf = (int64_t)tpol * nbls;
        const int64_t blk = (int64_t)nf * nt * per_tf;  // elements of one direction's output block
        // an earlier run may have the lanes busy
        FV_HIP(hipStreamSynchronize(stream));
        FV_HIP(hipStreamSynchronize(prep_stream));
        if (copy_stream) FV_HIP(hipStreamSynchronize(copy_stream));
        for (int li = 1; li < 4; ++li)
            if (lanes[li].stream && lanes[li].own_stream) FV_HIP(hipStreamSynchronize(lanes[li].stream));
        const int64_t d_elems = (int64_t)ndir * nant_basis * nbasis * (int64_t)freqs.size();
        const cplx<T> *dd = (const cplx<T> *)dcoefs;
        if (!dcoefs_on_device) {
            upload(d_bt_d, dcoefs, sizeof(cplx<T>) * (size_t)d_elems, 0);
            dd = d_bt_d.as<cplx<T>>();
        }
        {  // a value that is not finite fails the call before anything runs
            hipLaunchKernelGGL(k_count_nonfinite_c<T>, dim3((unsigned)std::min<int64_t>(cdiv(d_elems, 256), 4096)), dim3(256), 0,
                               stream, dd, d_elems, d_err.as<int>() + 4);
            int bad = 0;
            FV_HIP(hipMemcpyAsync(&bad, d_err.as<int>() + 4, sizeof(int), hipMemcpyDeviceToHost, stream));
            FV_HIP(hipStreamSynchronize(stream));
            if (bad) {
                FV_HIP(hipMemsetAsync(d_err.as<int>() + 4, 0, sizeof(int), stream));
                FV_HIP(hipStreamSynchronize(stream));
                throw Error(FV_ERR_ARG, std::to_string(bad) + " entries of dcoefs are not finite");
            }
        }
        const size_t out_bytes = sizeof(cplx<T>) * (size_t)ndir * (size_t)blk;
        cplx<T> *dout = (cplx<T> *)out;
        if (!out_on_device) {
            d_bt_out.reserve(std::max<size_t>(out_bytes, 16));
            dout = d_bt_out.as<cplx<T>>();
        }
        FV_HIP(hipMemsetAsync(dout, 0, out_bytes, stream));  // terms, chunks and height terms all add
        if (blk > 0) {
            if (mhist_log.size() > 65536) mhist_log.clear();
            RunPlan r{t0, t1, f0, f1, nt, nf};
            r.bt_d = dd;
            r.bt_ndir = ndir;
            r.bt_stride = blk;
            source_box(r.xc, r.X);
            height_terms(r);
            pair_setup(r);
            grid_and_groups(r);
            light_classes(r);
            lane_schedule(r);
            lane_plans(r);
            r.ch = source_chunks(r.nlanes_used);
            lane_buffers(r);
            OutBlock o{};  // direction 0's block; the epilogue reaches the others by bt_stride
            o.out = nullptr;
            o.on_device = true;
            o.nt = nt;
            o.nf = nf;
            o.dout = dout;
            o.per_tf = per_tf;
            o.run = (int64_t)nt * per_tf;
            o.fs = o.run;
            o.bytes = sizeof(cplx<T>) * (size_t)blk;
            o.run_bytes = sizeof(cplx<T>) * (size_t)o.run;
            o.shared = false;
            o.drain = false;
            Drain dr;
            queue_units(r, o, dr);
        }
        if (!out_on_device && out_bytes) FV_HIP(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
        {  // the staged directions and output belong to this pass: beyond the keep limit they go back
            const char *ek = std::getenv("FFTVIS_HIP_ADJ_KEEP_BYTES");
            if ((double)(d_bt_d.cap + d_bt_out.cap) > (ek ? std::atof(ek) : 256.0 * 1024 * 1024)) {
                d_bt_d.release();
                d_bt_out.release();
            }
        }
        check_errors();
    }

    // beam x coherency strengths of one (frequency group, beam pair) for the lane's current sources
    void launch_strengths(Lane &L, const RunPlan &r, const Pair &pr, int fa, int nfg, int64_t M, const int *Mp, hipStream_t on,
                          int wt_k = 0, Nufft3<T> *plan = nullptr, int t = 0) {
        Nufft3<T> *nufft = plan ? plan : L.plan[0].get();
        const int D = r.D;
        RoctxRange rr("strengths");
        size_t e2 = ev_begin(TM_STRENGTHS, on);
        StrengthArgs sa{};
        sa.M = M;
        sa.nfg = nfg;
        sa.f_first = fa;
        sa.nfreq = nfreq_cat;
        sa.polarized = polarized;
        sa.pol_sky = pol_sky;
        sa.same_beam = pr.bi == pr.bj;
        sa.herm = pr.herm;
        sa.dim = D;
        sa.w = nufft->ker.w;
        for (int d = 0; d < 3; ++d) {
            sa.h[d] = nufft->geo.d[d].h;
            sa.btc[d] = d < D ? pr.box_c()[d] : 0.0;
            sa.na[d] = d < D ? nufft->geo.d[d].na : 1;
        }
        sa.bi = desc(pr.bi);
        sa.bj = desc(pr.bj);
        sa.wt_k = r.K ? wt_k : 0;
        sa.wt_zc = r.zc;
        sa.wt_inv = r.zh > 0 ? 1.0 / r.zh : 0.0;
        const int ntrans = nfg * (pr.herm ? 2 : tpol);
        if (r.nsets()) {  // the position adjoint's and the tangent's sets, each M * ntrans elements: moments, then the source side's
            cplx<T> *cs3 = nufft->strengths_buffer(r.nsets() * ntrans);
            const int64_t set_stride = (int64_t)nufft->M * ntrans;
            if (r.moments) {
                hipLaunchKernelGGL((beam_order == 3 ? k_strengths_moments<T, 3> : beam_order == 1 ? k_strengths_moments<T, 1>
                                                                                                : k_strengths_moments<T, 0>),
                                   dim3(cdiv((int64_t)M * nfg, 256)), dim3(256), 0, on, sa, Mp,
                                   nufft->perm.template as<int>(), L.d_srcidx.template as<int>(),
                                   L.d_az.template as<T>(), L.d_za.template as<T>(), d_flux.p, d_freqs.as<double>(),
                                   nufft->i0s.template as<int>(), nufft->fs.template as<T>(), cs3,
                                   (const T *)L.d_xyz.template as<T>(), set_stride);
            }
            if (r.tan_sets) {
                SrcAccArgs aa{};
                aa.M = M;
                aa.nfreq = nfreq_cat;
                aa.polarized = polarized;
                aa.pol_sky = pol_sky;
                aa.same_beam = pr.bi == pr.bj;
                aa.D = r.tan_D;
                aa.set_stride = set_stride;
                aa.vstride = nsrc;
                aa.bi = sa.bi;
                aa.bj = sa.bj;
                aa.rt = rots[t];
                aa.rp = rplane;
                aa.h = r.tan_h;
                // the vectors horizon_step read for this time step (run_source_adjoint's choice)
                const T *vec = !astroms.empty() ? L.d_enu.template as<T>()
                                                : ntimes_topo ? d_topo.as<T>() + (size_t)t * 3 * nsrc : d_eq.as<T>();
                hipLaunchKernelGGL((beam_order == 3 ? k_strengths_tangent<T, 3> : beam_order == 1 ? k_strengths_tangent<T, 1>
                                                                                                : k_strengths_tangent<T, 0>),
                                   dim3(cdiv((int64_t)M * nfg, 256)), dim3(256), 0, on, sa, aa, Mp,
                                   nufft->perm.template as<int>(), L.d_srcidx.template as<int>(),
                                   L.d_az.template as<T>(), L.d_za.template as<T>(), d_flux.p, d_freqs.as<double>(),
                                   nufft->i0s.template as<int>(), nufft->fs.template as<T>(),
                                   cs3 + (r.moments ? 3 : 0) * set_stride, (const T *)L.d_xyz.template as<T>(), vec,
                                   r.tan_dtopo + (size_t)(t - r.t0) * 3 * nsrc);
            }
            ev_end(e2, on);
            return;
        }
        cplx<T> *cs = nufft->strengths_buffer(ntrans);
        hipLaunchKernelGGL((beam_order == 3 ? k_strengths<T, 3> : beam_order == 1 ? k_strengths<T, 1> : k_strengths<T, 0>),
                           dim3(cdiv((int64_t)M * nfg, 256)), dim3(256), 0, on, sa, Mp,
                           nufft->perm.template as<int>(), L.d_srcidx.template as<int>(),
                           L.d_az.template as<T>(), L.d_za.template as<T>(), d_flux.p, d_freqs.as<double>(),
                           nufft->i0s.template as<int>(), nufft->fs.template as<T>(), cs,
                           (const T *)(L.d_xyz.template as<T>() + 2 * M));
        ev_end(e2, on);
    }

    BeamDesc desc(int b) const {
        FV_REQUIRE(b >= 0 && b < (int)beams.size(), "beam pair refers to a missing beam");
        const Beam &bm = beams[b];
        BeamDesc d{};
        d.kind = bm.kind;
        d.order = beam_order;
        d.diameter = bm.diameter;
        for (int i = 0; i < 8; ++i) d.js[i] = bm.js[i];
        d.ps = bm.ps;
        d.table = bm.table ? bm.table->p : nullptr;
        d.nfreq_tab = bm.nfreq_tab;
        d.nza = bm.nza;
        d.naz = bm.naz;
        d.za_max = bm.za_max;
        return d;
    }

    // Called where the host has just synchronised with the main stream: a run that met bad input fails
    // here instead of returning finite, wrong visibilities (finufft rejects such points up front).
    void check_errors() {
        int e[NERR] = {0, 0, 0, 0, 0};
        FV_HIP(hipMemcpyAsync(e, d_err.p, sizeof(e), hipMemcpyDeviceToHost, stream));
        FV_HIP(hipStreamSynchronize(stream));
        if (!e[0] && !e[1] && !e[2] && !e[3] && !e[4]) return;
        FV_HIP(hipMemsetAsync(d_err.p, 0, sizeof(e), stream));
        if (e[4])
            throw Error(FV_ERR_ARG, std::to_string(e[4]) + " entries of the adjoint's visibility-shaped input are NaN");
        if (e[3])
            throw Error(FV_ERR_INTERNAL, "the gather met " + std::to_string(e[3]) + " transform columns its column plan had left "
                                         "out: the visibilities of this run are invalid (FFTVIS_HIP_NO_COLUMN_PLAN=1 avoids the plan)");
        if (e[2])
            throw Error(FV_ERR_ARG, "more sources above the horizon than source_buffer allows (" +
                                        std::to_string(e[2]) + " did not fit): increase source_buffer");
        if (e[1])
            throw Error(FV_ERR_INTERNAL, "type-1 entry buffers overflowed (" + std::to_string(e[1]) +
                                             " entries dropped): the visibilities of this run are invalid");
        throw Error(FV_ERR_ARG, std::to_string(e[0]) +
                                    " source positions were NaN or outside the unit sphere's box (non-unit "
                                    "coord_mgr vectors?): the visibilities of this run are invalid");
    }
    void sync() override {
        FV_HIP(hipSetDevice(device));
        FV_HIP(hipStreamSynchronize(stream));
        if (timing_level) ev_collect();
        check_errors();
    }
    void reserve_mhist(size_t bytes) {
        // growing the buffer frees the counts earlier device-output runs left in it for stats(): fold them first
        if (bytes > d_mhist.cap) fold_mhist();
        d_mhist.reserve(bytes);
    }
    void fold_mhist() {
        // above-horizon counts were left on the device during run(); fold them into the statistics
        if (!mhist_log.empty()) {
            FV_HIP(hipSetDevice(device));
            std::vector<int> mh(d_mhist.cap / sizeof(int));
            FV_HIP(hipMemcpyAsync(mh.data(), d_mhist.p, sizeof(int) * mh.size(), hipMemcpyDeviceToHost, stream));
            FV_HIP(hipStreamSynchronize(stream));
            for (const auto &e : mhist_log) {
                if (e.first < 0 || e.first >= (int)mh.size()) continue;
                st[ST_ABOVE_HORIZON] += mh[e.first];
                st[ST_SOURCE_VISITS] += (double)mh[e.first] * e.second;
                st[ST_MAX_ABOVE_HORIZON] = std::max(st[ST_MAX_ABOVE_HORIZON], (double)mh[e.first]);
            }
            mhist_log.clear();
        }
    }
    void stats(double *v, int n) override {
        fold_mhist();
        for (int i = 0; i < n && i < (int)(sizeof st / sizeof *st); ++i) v[i] = st[i];
    }
    void reset_stats() override {
        for (double &x : st) x = 0;
        for (double &x : tm) x = 0;
        spread_timed = 0;
        mhist_log.clear();
        ev_used = 0;
    }
    void enable_timing(int level) override { timing_level = level; }
    void timing(double *ms, int n) override {
        for (int i = 0; i < n && i < TM_COUNT; ++i) ms[i] = tm[i];
        if (n > TM_COUNT) ms[TM_COUNT] = spread_timed;
    }
};

}  // namespace fv
