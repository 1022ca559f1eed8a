/* fftvis_hip.h -- C ABI of libfftvis_hip.so, the MI355X (gfx950) backend that fills the
 * reference's stubbed `gpu` backend (tyler-a-cox/fftvis, src/fftvis/gpu/).
 *
 * Plain C, plain pointers and sizes; no C++/torch types cross this boundary.  Every entry point
 * returns an int status (0 = OK, see FV_* below); no exception crosses the ABI.  After a
 * non-zero status fv_last_error() returns a message owned by the library, valid until the next
 * failing call on the same host thread.  Host arrays are caller-owned, contiguous, never
 * modified; complex data is interleaved (re, im).  "precision" is the reference's:
 * 1 = float32/complex64, 2 = float64/complex128 (src/fftvis/cpu/cpu_simulate.py:591-596).
 *
 * Each declaration cites the reference interface it stands behind.
 */
#ifndef FFTVIS_HIP_H
#define FFTVIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV_OK 0
#define FV_ERR_ARG 1
#define FV_ERR_HIP 2
#define FV_ERR_ROCFFT 3 /* reserved (library FFT no longer used) */
#define FV_ERR_INTERNAL 4

/* ---- discovery / diagnostics ------------------------------------------------------------ */
int fv_version(void);                 /* 10000*major + 100*minor + patch */
int fv_device_count(int *count);      /* number of visible HIP devices (0 on a CPU-only box) */
int fv_device_bytes(int64_t *bytes);  /* device memory this process's handles hold right now (all devices) */
/* ... and the share of it on `device`: what the next run there reuses (its cached handle's buffers) -- the term the
 * host side adds to the free memory when it sizes chunks and blocks (wrapper.py:292-302 measures free host RAM).  */
int fv_device_bytes_on(int device, int64_t *bytes);
/* Free / total device memory of `device` (hipMemGetInfo): what the host side sizes its (time, frequency)
 * output blocks and source chunks against -- the device counterpart of the reference's
 * psutil.virtual_memory().available in simulate_vis (src/fftvis/wrapper.py:292-302).                 */
int fv_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes);
/* fv_nufft3 / fv_nudft3_direct keep a stream, device buffers and a plan per host thread between calls
 * (while the process holds < FFTVIS_HIP_HANDLE_CACHE_BYTES, default 2 GiB, of device memory): this frees
 * them all, including those of threads that have exited.  Call it while no transform is in flight. */
int fv_release_workspaces(void);
const char *fv_last_error(void);

/* ---- standalone type-3 NUFFT ---------------------------------------------------------------
 * out[t][k] = sum_j c[t][j] exp(+i (s_k x_j + t_k y_j [+ u_k z_j])),   relative l2 error ~ eps.
 * Replaces: gpu_nufft2d / gpu_nufft3d stubs  (src/fftvis/gpu/nufft.py:11-50, 53-98), i.e. the
 * GPU twins of cpu_nufft2d / cpu_nufft3d -> finufft.nufft2d3 / nufft3d3
 * (src/fftvis/cpu/nufft.py:48-59, 105-118; modeord irrelevant for type 3, isign = +1 default).
 * dim = 2: z and u must be NULL.  x,y,z: (M) reals; c: (ntrans, M) complex; s,t,u: (N) reals;
 * out: (ntrans, N) complex, caller-allocated.  upsampfac in {2.0, 1.25}
 * (cpu/nufft.py:19 "upsample_factor"); 1.25 reaches ~1e-8 at best in fp64 (kernel one cell wider
 * than finufft's formula, capped at 15: beyond that amplified rounding at band-edge targets
 * outweighs the truncation gain).  Host pointers.  NaN / infinite source coordinates are refused
 * (FV_ERR_ARG), as finufft refuses them.                                                      */
int fv_nufft3(int device, int precision, int dim, int64_t M, const void *x, const void *y,
              const void *z, const void *c, int ntrans, int64_t N, const void *s, const void *t,
              const void *u, double eps, double upsampfac, void *out);

/* Same transform by brute force on the GPU (O(M N) direct sum in fp64 accumulators): an
 * independent device-side check used by the parity tests at sizes the CPU oracle cannot reach. */
int fv_nudft3_direct(int device, int precision, int dim, int64_t M, const void *x, const void *y,
                     const void *z, const void *c, int ntrans, int64_t N, const void *s,
                     const void *t, const void *u, void *out);

/* ---- stand-alone pieces of the slice (the other stubbed GPU entry points) -----------------
 * Host pointers; real/complex of `precision`.
 *
 * fv_beam_eval: GPUBeamEvaluator.evaluate_beam (src/fftvis/gpu/beams.py:18-66; CPU twin
 * cpu/beams.py:12-89).  kind/diameter/table as in fv_sim_set_beam_*; out is (2,2,n) complex
 * [ax][feed][src] when polarized, else (n) complex power.  For kind 0 a non-NULL `table` holds 9
 * float64: the four complex Jones factors and the power factor of fv_sim_set_beam_airy_scaled.
 * fv_apparent_coherency: GPUBeamEvaluator.get_apparent_flux_polarized (gpu/beams.py:68-88) and
 * its CPU siblings (cpu/beams.py:129-246, cpu_simulate.py:183-187); variant 0..4:
 *   0 (A^H A) I   1 A^H C A   2 Ai^H Aj I   3 Ai^H C Aj   4 sqrt(Bi Bj) I (1-D arrays).
 *   beam_i/beam_j/out: (2,2,n) complex (variant 4: (n)); flux: (n) real or (2,2,n) complex.
 * fv_inplace_rot: gpu.utils.inplace_rot (src/fftvis/gpu/utils.py:8-22): b (3,n) <- rot (3,3) b. */
int fv_beam_eval(int device, int precision, int polarized, int kind, double diameter,
                 int nfreq_tab, int nza, int naz, double za_max, const void *table, int order,
                 int freq_index, double freq, int64_t n, const void *az, const void *za, void *out);
int fv_apparent_coherency(int device, int precision, int variant, int64_t n, const void *beam_i,
                          const void *beam_j, const void *flux, void *out);
/* fv_residual_chi2: the residual step of a fit on its own (the kernel pair fv_sim_run_residual queues behind its forward
 * run).  vis, data: (nrows, row_len) complex of `precision`, C-contiguous; weights: (nrows, row_len) real of `precision`,
 * or NULL (every weight 1).  In place  vis <- G = 2 w (vis - data):  delta = vis - data and G = 2 w delta in that
 * precision (two roundings and an exact doubling).  chi2_rows[i] = sum over row i of w |delta|^2 with every term formed
 * and added in fp64: per block of the row an __shfl_xor tree and a pass through LDS, the blocks' partials then added in
 * index order -- no floating-point atomics, the same input gives the same bits.  A weight of exactly 0 flags its sample:
 * G is exactly 0 there, nothing is added and the datum is not used (NaN or Inf there do not propagate).  A weight that
 * is negative or not finite, and a datum that is not finite where the weight is positive, are counted in the same pass
 * and fail the call with FV_ERR_ARG and a message that says which; vis and chi2_rows are then invalid.  Host pointers. */
int fv_residual_chi2(int device, int precision, int64_t nrows, int64_t row_len, void *vis, const void *data,
                     const void *weights, double *chi2_rows);
/* fv_gain_residual_chi2: fv_residual_chi2 with one complex gain per antenna and feed folded in (the kernels
 * fv_sim_run_residual_gains queues behind its forward run).  vis, data, weights: nrows rows of tpol nbls values, element
 * e of a row has pol = e / nbls and baseline k = e % nbls = (ant1[k], ant2[k]); gains: (nrows, nfeed, nant) complex of
 * `precision`, nfeed = 1 for tpol = 1 and 2 for tpol = 4.  Of the two feed axes of a polarized row the minor one is the
 * first antenna's: pol = 2 q + p, p the feed of ant1[k] and q of ant2[k].  Per element, in that precision and this order,
 *   m = conj(g[p, ant1]) g[q, ant2],  V' = m vis,  delta = V' - data,  G' = 2 (w delta),  vis <- G = conj(m) G' = d chi2 / dV,
 * chi2_rows[i] = sum over row i of w |delta|^2, formed, added and reduced as fv_residual_chi2 does, with its rules for
 * flagged samples and bad input.  ggains: (nrows, nfeed, nant) complex128, or NULL (its kernel does not run):
 *   ggains[i, f, a] = sum_{k: ant1[k] = a, p = f} conj(G') g[q, ant2] V  +  sum_{k: ant2[k] = a, q = f} G' g[p, ant1] conj(V),
 * d chi2 = Re sum conj(ggains) dg, every term formed in fp64 from the inputs of `precision` and added in fp64 over the
 * antenna's incidence list (ascending k, "a is ant1" first) by one wave with a fixed lane <-> entry assignment and an
 * __shfl_xor tree -- no floating-point atomics; an antenna without a baseline gets exactly 0.  tpol not in {1, 4}, an
 * antenna index outside [0, nant) and a null gains fail with FV_ERR_ARG before anything runs.  Host pointers. */
int fv_gain_residual_chi2(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                          const int *ant2, const void *gains, void *vis, const void *data, const void *weights,
                          double *chi2_rows, void *ggains);
/* fv_jones_residual_chi2: fv_residual_chi2 with one 2 x 2 complex (Jones) matrix per antenna folded in: leakage between the
 * feeds as well as their gains (the kernels fv_sim_run_residual_jones queues behind its forward run).  vis, data, weights:
 * nrows rows of 4 nbls values, value pol nbls + k of a row is V[x, y] of baseline k = (ant1[k], ant2[k]), pol = 2 x + y, y
 * the feed of ant1[k] (the conjugated antenna) and x of ant2[k], as for fv_gain_residual_chi2.  jones: (nrows, 2, 2, nant)
 * complex of `precision`, jones[r, i, j, a] = Gamma_a[i, j] with i the feed of the ideal antenna and j the measured one:
 * antenna a's Jones matrix A_a[ax, feed] becomes A_a Gamma_a, and Gamma_a = diag(g[a]) are fv_gain_residual_chi2's gains.
 * With G1 = Gamma[ant1[k]] and G2 = Gamma[ant2[k]], per baseline,
 *   V'[x, y]  = sum_{x', y'} conj(G1[y', y]) G2[x', x] V[x', y'],   delta = V' - data,   G'[x, y] = 2 w[x, y] delta[x, y],
 *   vis <- G[x', y'] = sum_{x, y} conj(G2[x', x]) G'[x, y] G1[y', y] = d chi2 / dV,
 * chi2_rows[i] = sum over row i of w |delta|^2.  In that precision every operation rounds on its own, in this order, each
 * sum of two products left to right:
 *   B[x', y] = V[x', 0] conj(G1[0, y]) + V[x', 1] conj(G1[1, y]),     V'[x, y]  = G2[0, x] B[0, y] + G2[1, x] B[1, y],
 *   delta = V' - data,   G' = 2 (w delta),
 *   C[x', y] = conj(G2[x', 0]) G'[0, y] + conj(G2[x', 1]) G'[1, y],   G[x', y'] = C[x', 0] G1[y', 0] + C[x', 1] G1[y', 1],
 * so that identity matrices give fv_residual_chi2's bits, in vis and in chi2_rows: the row terms are formed as there and
 * added in its order (they pass through an fp64 block of the rows' shape on the device) -- no floating-point atomics, the
 * same input gives the same bits.  A weight of exactly 0 flags that one (x, y) sample: G' is exactly 0 there, the datum is
 * not used (NaN or Inf there do not propagate), nothing is added to chi2_rows or gjones, and the baseline's other samples
 * still use all four model values; a baseline with all four samples flagged stores G = 0 exactly.  Bad weights and data
 * are counted and reported as fv_residual_chi2 does.  gjones: (nrows, 2, 2, nant) complex128, or NULL (its kernel does
 * not run):
 *   gjones[r, y', y, a] += sum_x conj(G'[x, y]) (G2^T V)[x, y']      for every k with ant1[k] = a,
 *   gjones[r, x', x, a] += sum_y G'[x, y] conj((V conj G1)[x', y])   for every k with ant2[k] = a,
 * d chi2 = Re sum conj(gjones) dGamma (an auto-correlation adds to both), every term formed in fp64 from the inputs of
 * `precision` and added in fp64 over the antenna's incidence list (ascending k, "a is ant1" first) by one wave per (row,
 * antenna) that holds all four entries, with a fixed lane <-> entry assignment and an __shfl_xor tree; an antenna without
 * a baseline gets exactly 0.  An antenna index outside [0, nant) and a null jones fail with FV_ERR_ARG before anything
 * runs.  Host pointers. */
int fv_jones_residual_chi2(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1,
                           const int *ant2, const void *jones, void *vis, const void *data, const void *weights,
                           double *chi2_rows, void *gjones);
/* fv_gain_normal_rows: one evaluation of the normal sums of the gain solve (the gather fv_gain_solve iterates).  The rows,
 * the pairs and the feeds (pol = 2 q + p) are fv_gain_residual_chi2's; vis, data, weights are read only; gains:
 * (nrows, nfeed, nant) complex128 whatever `precision` is.  A sample is used when w > 0 and ant1[k] != ant2[k]: an
 * auto-correlation is quadratic in one gain and counts as flagged; a flagged sample is not read (NaN or Inf there do not
 * propagate).  For fixed V the least-squares problem in one antenna's gain, the others held, is linear, and its normal
 * sums over the used samples are, per row i, feed f and antenna a,
 *   side 0 (a = ant1[k], f = p, every q):  num += w g[q, ant2] V conj(d)      den += w |g[q, ant2]|^2 |V|^2
 *   side 1 (a = ant2[k], f = q, every p):  num += w g[p, ant1] conj(V) d      den += w |g[p, ant1]|^2 |V|^2
 * num: (nrows, nfeed, nant) complex128, den: the same shape in float64; with the autos flagged fv_gain_residual_chi2's
 * ggains = 2 (den g - num).  Every term is formed in fp64 from the inputs of `precision` and added in fp64 over the
 * antenna's incidence list as ggains is added (one wave, lane l takes entries l, l + 64, ..., an __shfl_xor tree) -- no
 * floating-point atomics, the same input gives the same bits; an antenna without a used sample gets exactly 0 in both.
 * tpol not in {1, 4}, a negative shape, nant < 1, an antenna index outside [0, nant) and a null pointer fail with
 * FV_ERR_ARG before anything runs.  Host pointers. */
int fv_gain_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, const void *gains, const void *vis, const void *data, const void *weights, void *num,
                        double *den);
/* fv_gain_solve: the gains that minimise sum w |conj(g[p, ant1]) g[q, ant2] V - d|^2 over the used samples for a FIXED
 * model V, by the alternating per-antenna solve (StefCal), entirely on the device.  vis, data, weights: the
 * (nfreqs, ntimes) rows (row = f ntimes + t, as fv_sim_run lays them out) of tpol nbls values of `precision`, each a host
 * block (staged once per call) or, with its on_device flag, a device block that is read where it lies and never
 * modified; weights may be NULL (every weight 1).  gains: host, complex128, (nfreqs, per_time ? ntimes : 1, nfeed, nant);
 * in: the start, out: the result.  A solve unit is a frequency for time-constant gains (per_time = 0) and a
 * (frequency, time) for per-time gains.  Iteration i = 1, 2, ...: the normal sums of fv_gain_normal_rows at the current
 * gains, for time-constant gains added over the unit's times in ascending order; g^ = num / den where den > 0 (an antenna
 * with den == 0 keeps its value and is not solved); g <- g^ for odd i and (g^ + g) / 2 for even i, written into the other
 * of two buffers; change[unit] = max |g_new - g| / max |g_new| over the unit's feeds and antennas.  The loop ends after
 * the first iteration at which every unit has change < tol, or at max_iter; every unit iterates until then (tol = 0 runs
 * exactly max_iter iterations).  The iterate is complex128 on the device and only the units' change comes to the host per
 * iteration.  niter_out: the iterations run; change_out: (units) the last iteration's change; chi2_ft_out:
 * (nfreqs, ntimes) sum w |V' - d|^2 over the used samples at the returned gains, from one more pass of the gather over
 * each antenna's side-0 entries (every baseline once) and a per-row sum in a fixed order; solved_out: int32 in gains'
 * shape, 0 where den == 0 at the last iteration.  The common phase is left where the iteration puts it.  One counting
 * pass before the loop fails the call with FV_ERR_ARG for a weight that is negative or not finite and a datum that is not
 * finite at a used sample (fv_residual_chi2's messages) and for a model value that is not finite; gains is then
 * untouched.  tpol not in {1, 4}, a negative shape, nant < 1, an antenna index outside [0, nant), a null pointer, a flag
 * that is not 0 or 1, max_iter < 1 and a negative or NaN tol fail with FV_ERR_ARG before anything runs.  nbls == 0: the
 * start gains, chi2 0, nothing solved, niter 0. */
int fv_gain_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                  const int *ant2, int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device,
                  const void *weights, int weights_on_device, void *gains, int max_iter, double tol, int *niter_out,
                  double *change_out, double *chi2_ft_out, int *solved_out);
/* fv_redundant_vis_rows: the visibility step (U-step) of redundant calibration on its own: the weighted average of the
 * calibrated data over every redundant group, at fixed gains.  The rows, the pairs and the feeds (pol = 2 q + p) are
 * fv_gain_normal_rows'; group: (nbls) int32, the redundant group of baseline k, in [0, ngroups); gains: (nrows, nfeed,
 * nant) complex128 whatever `precision` is; data, weights: read only, weights may be NULL (every weight 1).  The data
 * model is V'[row, pol, k] = conj(g[p, ant1]) g[q, ant2] U[row, pol, group[k]], one unknown visibility U per row, pol and
 * group.  A sample is used when w > 0 and ant1[k] != ant2[k]; a flagged datum is not read (NaN or Inf there do not
 * propagate).  With m = conj(g[p, ant1]) g[q, ant2], over the used samples of group r,
 *   num = sum w conj(m) d      den = sum w |m|^2      U = num / den where den > 0, else U keeps its value
 * uvis: (nrows, tpol, ngroups) complex128, in: the values a group without a used sample keeps, out: U; den: the same
 * shape in float64.  Every term is formed in fp64 from the inputs of `precision` and added in fp64 over the group's
 * members in ascending k by one wave per (row, group) (lane l takes members l, l + 64, ..., all tpol samples of a member,
 * an __shfl_xor tree) -- no floating-point atomics, the same input gives the same bits.  The baselines carry no flip: a
 * baseline measured in the opposite orientation is swapped and its datum conjugated by the caller.  tpol not in {1, 4}, a
 * negative shape, nant < 1, ngroups < 1, an antenna index outside [0, nant), a group index outside [0, ngroups) and a
 * null pointer fail with FV_ERR_ARG before anything runs; nbls == 0 returns den = 0 and leaves uvis.  Host pointers. */
int fv_redundant_vis_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                          const int *ant2, int ngroups, const int *group, const void *gains, const void *data,
                          const void *weights, void *uvis, double *den);
/* fv_redundant_normal_rows: the gain step's gather of redundant calibration on its own: fv_gain_normal_rows with the model
 * V = U[row, pol, group[k]] read from uvis, (nrows, tpol, ngroups) complex128, in place of a block vis.  The order of the
 * sums, the flags and the outputs num, den (nrows, nfeed, nant) are fv_gain_normal_rows'; group and the argument checks are
 * fv_redundant_vis_rows'.  Host pointers. */
int fv_redundant_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                             const int *ant2, int ngroups, const int *group, const void *gains, const void *uvis,
                             const void *data, const void *weights, void *num, double *den);
/* fv_redundant_solve: redundant calibration, entirely on the device: the gains g and the group visibilities U that minimise
 * sum w |conj(g[p, ant1]) g[q, ant2] U[row, pol, group[k]] - d|^2 over the used samples, without a sky model.  data,
 * weights, gains, per_time and the solve units are fv_gain_solve's; group is fv_redundant_vis_rows'.  U is per row even
 * when the gains are time-constant, and starts from 0.  Iteration i = 1, 2, ...: the U-step of fv_redundant_vis_rows at
 * the current gains; then the normal sums of fv_redundant_normal_rows at these U, for time-constant gains added over the
 * unit's times in ascending order, and fv_gain_solve's update: g^ = num / den where den > 0, g <- g^ for odd i and
 * (g^ + g) / 2 for even i, change[unit] = max |g_new - g| / max |g_new|.  The loop ends as fv_gain_solve's does, and only
 * the units' change comes to the host per iteration.  After the loop one more U-step at the returned gains, and chi2 at
 * (g, U) as fv_gain_solve forms it.  uvis_out: host, complex128, (nfreqs, ntimes, tpol, ngroups); vis_solved_out: int32 in
 * the same shape, 0 where the group had no used sample in that row and pol (U is 0 there); niter_out, change_out,
 * chi2_ft_out, solved_out: fv_gain_solve's.  Four degrees of freedom per unit and feed are not constrained by the data
 * (amplitude, phase and a phase gradient across the array) and are left where the iteration puts them.  The counting pass
 * of fv_gain_solve, without a model, fails the call with its messages; gains is then untouched.  The argument checks are
 * fv_gain_solve's and fv_redundant_vis_rows'.  nbls == 0: the start gains, U = 0, chi2 0, nothing solved, niter 0. */
int fv_redundant_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                       const int *ant2, int ngroups, const int *group, int per_time, const void *data, int data_on_device,
                       const void *weights, int weights_on_device, void *gains, void *uvis_out, int max_iter, double tol,
                       int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, int *vis_solved_out);
/* fv_firstcal_pair_delays: stage 1 of firstcal, the start of fv_redundant_solve on data whose gains carry cable delays:
 * the delay difference of every pair of baselines of one redundant group.  The block, the weights and the on_device flags
 * are fv_redundant_solve's; pair1, pair2: (npairs) int32, the baselines k and k' of pair i, both of one group (the caller
 * takes consecutive members of every group); ant1, ant2 only tell which baselines are auto-correlations.  Feed p of a
 * polarized block uses the parallel hand pol = 3 p.  A sample is used when w > 0 and ant1[k] != ant2[k]: weights act as
 * flags here, and a flagged datum is not read.  The group's visibility cancels out of
 *   z[feed, i, f] = sum_t d[f, t, pol, k] conj(d[f, t, pol, k'])      over the times at which both samples are used
 * every term formed and added in fp64, times ascending.  With ND = pad nfreqs the coarse peak is the lowest n of maximal
 * |P[n]|^2, P[n] = sum_f z[f] exp(-2 pi i n f / ND), n = 0 .. ND - 1, taken as a signed bin: n - ND where 2 n >= ND.  Four
 * rounds of a parabola through |P(x)|^2 at x - h, x, x + h, h = 1, 1/4, 1/16, 1/64, evaluated at the continuous x, refine
 * it: den = y- - 2 y0 + y+, and where den < 0 the step 0.5 h (y- - y+) / den clipped to +-h.  One wave per (feed, pair):
 * the bins go over the lanes with twiddles exp(-2 pi i j / ND) built on the host in fp64 and indexed by n f mod ND; the
 * refinement uses sincospi in fp64 with the lanes splitting the sum over f and a fixed __shfl_xor tree -- no
 * floating-point atomics, the same input gives the same bits.  Outputs, host, (nfeed, npairs): peak_bin_out int32, the signed
 * coarse bin; delay_bins_out float64, the refined x in bins (the pair's delay tau[a2[k]] - tau[a1[k]] - tau[a2[k']] +
 * tau[a1[k']] is x / (ND dnu): the library needs no channel width; beyond +-ND / 2 it aliases); power_out, |P(x)|^2;
 * total_out, sum_f |z[f]|^2; used_out int32, 1 when at least two channels have a non-zero z, else 0 with bin 0, x = 0 and
 * power 0.  tpol not in {1, 4}, a negative shape, pad < 1 or pad nfreqs >= 2^20, an on_device flag outside {0, 1}, a
 * baseline index outside [0, nbls) and a null pointer fail with FV_ERR_ARG before anything runs; npairs == 0 is a valid
 * call, and nbls == 0, nfreqs == 0 or ntimes == 0 return zeros. */
int fv_firstcal_pair_delays(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int npairs, const int *pair1,
                            const int *pair2, const int *ant1, const int *ant2, const void *data, int data_on_device,
                            const void *weights, int weights_on_device, int pad, int *peak_bin_out, double *delay_bins_out,
                            double *power_out, double *total_out, int *used_out);
/* fv_firstcal_offsets: stage 2 of firstcal: one complex number per antenna and feed, constant in frequency and time, on
 * the block derotated by the delay model.  slopes: host, (nfeed, nant) float64, s = 2 pi tau dnu in radians per channel;
 *   d'[f, t, pol, k] = d exp(-i (f - (nfreqs - 1) / 2) (s[q, ant2] - s[p, ant1]))      p = pol & 1, q = pol >> 1
 * with the phase and the product in fp64, written into a buffer of the call: the caller's data are never written, and a
 * flagged datum is not read.  fv_redundant_solve's loop then runs on d' with the whole block as one solve unit, U per row.
 * offsets: host, (nfeed, nant) complex128, in: the start, out: the result; change_out: one value; uvis_out, niter_out,
 * chi2_ft_out (nfreqs, ntimes), solved_out (nfeed, nant), vis_solved_out, max_iter, tol, the counting pass, its messages
 * and the argument checks are fv_redundant_solve's.  nbls == 0: the start, U = 0, chi2 0, nothing solved, niter 0. */
int fv_firstcal_offsets(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, int ngroups, const int *group, const double *slopes, const void *data, int data_on_device,
                        const void *weights, int weights_on_device, void *offsets, void *uvis_out, int max_iter, double tol,
                        int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, int *vis_solved_out);
/* fv_abscal_slopes: absolute calibration of a redundant solve: the amplitude and the phase gradient the data leave free,
 * fitted to a model of the group visibilities.  uvis (complex128), model (complex64 / complex128 by precision) and gweights
 * (float64, null: ones) are (nfreqs, ntimes, tpol, ngroups) blocks, fv_redundant_solve's layout of uvis_out, each on the host
 * or, with its on_device flag 1, on `device`; all three are read only.  A solve unit is a frequency (per_time 0: the sums run
 * over its ntimes times) or a (frequency, time) (per_time 1); a row is a (unit, feed), nfeed = 2 for tpol 4, and feed p reads
 * the parallel hand pol = 3 p.  coords: host, (ngroups, ndim) float64, the groups' baselines X_g in in-plane coordinates, ndim
 * 1 (a line) or 2.  A sample is used when W > 0 and X_g != 0 (an auto-correlation's own group is never used); a flagged datum
 * is not read.  Per row, every term formed and added in fp64, times ascending,
 *   c_g = sum_t W conj(U) M,   N = sum W |U|^2,   P = sum W |M|^2,   S(Phi) = sum_g c_g exp(i Phi . X_g)
 * and chi2(eta, Phi) = sum W |eta exp(-i Phi . X_g) U - M|^2 is least where Re S(Phi) is largest, with eta = Re S / N.  The
 * search evaluates Re S on the grid Phi = (j_1 h1, j_2 h2), j_i = i_i - (n_i - 1) / 2, i_i = 0 .. n_i - 1 (n2 = 1 for ndim 1) and
 * takes the point of the largest value, on a tie the lowest flat index i_1 n2 + i_2: the phase Phi . X in fp64, one sincos at
 * the first point of a run of 8 consecutive grid points followed by 7 rotations by exp(i h X), the groups added in
 * ascending order.  `refine` rounds of Newton on Re S follow, at the continuous Phi with sincos in fp64: with the gradient
 * g = -sum X Im(c e^{i Phi . X}) and the Hessian H = -sum X X^T Re(c e^{i Phi . X}) the step is -H^-1 g where H is negative
 * definite, else g / max |eig H| (0 where H = 0), either clipped to +-h_i per dimension; one more evaluation at the result gives
 * Re S.  No floating-point atomics: the same input gives the same bits.  Outputs, host, (nunits, nfeed, ...): peak_out int32
 * (.., 2), the grid point (j_1, j_2); slopes_out float64 (.., 2), the refined in-plane Phi; amp_out, eta; power_out, Re S;
 * unorm_out, N; mnorm_out, P; used_out int32, 1 when N > 0, at least ndim + 1 groups have a used sample and Re S > 0, else 0
 * with eta = 1, Phi = 0, the peak (0, 0) and power 0; chi2_ft_out (nfreqs, ntimes) float64, sum W |eta exp(-i Phi . X) U - M|^2
 * over the feeds and the used samples, formed explicitly at the returned parameters.  A negative or non-finite weight, and a
 * non-finite value of uvis or model at a used sample, fail the call with FV_ERR_ARG (fv_redundant_solve's messages).  tpol
 * not in {1, 4}, a negative shape, per_time outside {0, 1}, ndim outside {1, 2}, n1 or n2 even or not positive, n1 n2 above
 * 2^22, n2 != 1 for ndim 1, a step that is not positive and finite, refine outside 0 .. 32, an on_device flag outside {0, 1},
 * coords that are not finite and a null pointer fail with FV_ERR_ARG before anything runs; ngroups == 0, nfreqs == 0 and
 * ntimes == 0 give the neutral result: eta = 1, everything else 0. */
int fv_abscal_slopes(int device, int precision, int nfreqs, int ntimes, int tpol, int ngroups, int per_time, const void *uvis,
                     int uvis_on_device, const void *model, int model_on_device, const void *gweights, int gweights_on_device,
                     const double *coords, int ndim, int n1, int n2, double h1, double h2, int refine, int *peak_out,
                     double *slopes_out, double *amp_out, double *power_out, double *unorm_out, double *mnorm_out, int *used_out,
                     double *chi2_ft_out);
/* fv_abscal_evaluate: the evaluation fv_abscal_slopes' refinement iterates, alone, at the caller's slopes.  All host: c
 * (nrows, ngroups) complex128, the rows' strengths; coords (ngroups, ndim) float64; slopes (nrows, 2) float64 (the second
 * ignored for ndim 1: x_2 = 0); out (nrows, 6) float64: f = Re S, g_1, g_2, H_11, H_12, H_22 with
 *   S = sum_g c_g exp(i Phi . X_g),   g = -sum X Im(c e^{i Phi . X}),   H = -sum X X^T Re(c e^{i Phi . X}),
 * one wave per row, lane l adding the groups l, l + 64, ... and a fixed __shfl_xor tree.  A negative shape, ndim outside
 * {1, 2}, coords that are not finite and a null pointer fail with FV_ERR_ARG before anything runs; nrows == 0 is a valid call
 * and ngroups == 0 returns zeros. */
int fv_abscal_evaluate(int device, int nrows, int ngroups, const void *c, const double *coords, int ndim, const double *slopes,
                       double *out);
/* fv_jones_normal_rows: one evaluation of the 2 x 2 normal systems of the Jones solve (the gather fv_jones_solve
 * iterates).  The rows, the pairs and the layout of the matrices are fv_jones_residual_chi2's; vis, data, weights are
 * read only; jones: (nrows, 2, 2, nant) complex128 whatever `precision` is.  A sample is used when w > 0 and
 * ant1[k] != ant2[k]; a flagged datum is not read, and a baseline without a used sample is skipped before V is read.  For
 * fixed V the least-squares problem in one antenna's matrix, the others held, is linear and splits into one Hermitian
 * 2 x 2 system per measured feed (column) c of Gamma_a.  With G1 = Gamma[ant1[k]], G2 = Gamma[ant2[k]],
 *   side 1 (a = ant2[k], c = x), Z[x', y] = sum_{y'} V[x', y'] conj(G1[y', y]):
 *     A[i, j] += w[x, y] conj(Z[i, y]) Z[j, y]      b[i] += w[x, y] conj(Z[i, y]) d[x, y]      summed over y
 *   side 0 (a = ant1[k], c = y), Y[x, y'] = sum_{x'} G2[x', x] V[x', y']:
 *     A[i, j] += w[x, y] Y[x, i] conj(Y[x, j])      b[i] += w[x, y] Y[x, i] conj(d[x, y])      summed over x
 * A_out: (nrows, 4, 2, nant) float64 = [A00, A11, Re A01, Im A01] x column x antenna; b_out: (nrows, 2, 2, nant)
 * complex128, [i, column, a]; with the autos flagged fv_jones_residual_chi2's gjones[:, c, a] = 2 (A Gamma_a[:, c] - b).
 * Every term is formed in fp64 from the inputs of `precision` and added in fp64 over the antenna's incidence list as
 * gjones is added (one wave per (row, antenna), lane l takes entries l, l + 64, ..., an __shfl_xor tree) -- no
 * floating-point atomics, the same input gives the same bits; an antenna without a used sample gets exactly 0 in both.
 * A negative shape, nant < 1, an antenna index outside [0, nant) and a null pointer fail with FV_ERR_ARG before anything
 * runs; nrows or nbls == 0 return zeros.  Host pointers. */
int fv_jones_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                         const void *jones, const void *vis, const void *data, const void *weights, double *A_out, void *b_out);
/* fv_jones_solve: the 2 x 2 matrices that minimise sum w |V' - d|^2, V' = G2^T V conj(G1), over the used samples for a
 * FIXED polarized model V, by the alternating per-antenna solve (StefCal for full Jones matrices), entirely on the
 * device.  fv_gain_solve argument for argument, without tpol (the rows hold 4 nbls values).  jones: host, complex128,
 * (nfreqs, per_time ? ntimes : 1, 2, 2, nant); in: the start, out: the result.  Iteration i = 1, 2, ...: the systems of
 * fv_jones_normal_rows at the current matrices, for time-constant matrices added over the unit's times in ascending
 * order; a column is solved when A00 > 0, A11 > 0 and det = A00 A11 - |A01|^2 > 2^-30 A00 A11, else both of its entries
 * keep their values; Gamma^[:, c] = A^-1 b by the closed form; Gamma <- Gamma^ for odd i and (Gamma^ + Gamma) / 2 for even
 * i, written into the other of two buffers; change[unit] = max |new - old| / max |new| over the unit's 4 nant entries.
 * The loop ends as fv_gain_solve's does.  niter_out, change_out, chi2_ft_out: as there, chi2 at the returned matrices;
 * solved_out: int32 (units, 2, nant), per column and antenna, at the last iteration.  The counting pass, its messages
 * and the argument checks are fv_gain_solve's; jones is untouched when the call fails.  nbls == 0: the start matrices,
 * chi2 0, nothing solved, niter 0. */
int fv_jones_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int nant, const int *ant1, const int *ant2,
                   int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device, const void *weights,
                   int weights_on_device, void *jones, int max_iter, double tol, int *niter_out, double *change_out,
                   double *chi2_ft_out, int *solved_out);
/* fv_weight_rows: the weighting step of a Gauss-Newton product on its own (the kernel pair fv_sim_weight_block queues).
 * parts: nparts = 1 .. 4 blocks P_0 .. P_{nparts-1}, each (nrows, row_len) complex of `precision`, C-contiguous -- the
 * parts of a tangent J p; weights: (nrows, row_len) real of `precision`, or NULL (every weight 1).  Per element, in that
 * precision and in this order:  U = ((P_0 + P_1) + P_2) + P_3  (component-wise, only the parts given),  G = 2 (w U)  (one
 * rounding per component and an exact doubling), written in place into parts[0] (the other parts are read only);
 * q_rows[i] = sum over row i of w |U|^2 with every term formed and added in fp64, reduced as fv_residual_chi2 reduces --
 * no floating-point atomics, the same input gives the same bits.  A weight of exactly 0 flags its sample: G is exactly 0
 * there, nothing is added and the parts are not used (NaN or Inf there do not propagate).  A weight that is negative or
 * not finite is counted in the same pass and fails the call with FV_ERR_ARG and fv_residual_chi2's message; parts[0] and
 * q_rows are then invalid.  nparts outside 1 .. 4, a null part and a null q_rows with nrows > 0 fail with FV_ERR_ARG
 * before anything runs.  Host pointers. */
int fv_weight_rows(int device, int precision, int64_t nrows, int64_t row_len, int nparts, const void *const *parts,
                   const void *weights, double *q_rows);
/* fv_gain_weight_rows: fv_weight_rows with per-antenna gains and a gain direction folded in (the kernel pair
 * fv_sim_gain_weight_block queues): the weighting step of a Gauss-Newton product of fv_gain_residual_chi2's chi2.  The
 * rows, the pairs, the feeds (pol = 2 q + p) and gains are fv_gain_residual_chi2's; d_gains: the gain direction dg in
 * gains' layout, or NULL; parts: nparts = 0 .. 4 blocks as for fv_weight_rows (nparts = 0, the gains-only direction,
 * needs d_gains); vis: the forward V at the real parameters, needed with d_gains or hgains, else it may be NULL.  Per
 * element of baseline k = (a1, a2), with g1 = g[p, a1], g2 = g[q, a2], h1 = dg[p, a1], h2 = dg[q, a2] and
 * U = ((P_0 + P_1) + P_2) + P_3 (0 for nparts = 0), in `precision`, every operation rounded on its own, in this order:
 *   m  = conj(g1) g2                     dm = conj(h1) g2 + conj(g1) h2      (dm = 0 without a gain direction)
 *   U' = m U + dm V                      (the tangent of V' along p = (sky directions, dg))
 *   G' = 2 (w U')                        quad row += w |U'|^2  (terms formed and added in fp64)
 *   stored G = conj(m) G'                (what the public sky adjoints read: their result on it is H p for their block)
 *   hgains[a, f] = sum_{k: a1=a, p=f} conj(G') g2 V  +  sum_{k: a2=a, q=f} G' g1 conj(V)
 * G is written in place into parts[0], or into vis for nparts = 0 (everything else is read only); q_rows[i] is row i's
 * sum, reduced as fv_residual_chi2 reduces; over all rows <p, H p> = 2 sum q_rows, the gains' inner product being
 * Re sum conj(dg) hgains.  hgains: (nrows, nfeed, nant) complex128, the gain block of H p in the convention of ggains, or
 * NULL (its kernel does not run); every term is formed in fp64 from the inputs of `precision` (U' = m U + dm V and G' in
 * fp64) and added as fv_gain_residual_chi2 adds ggains -- no floating-point atomics, the same input gives the same
 * bits; an antenna without a baseline gets exactly 0.  With unit gains and no direction G and q_rows are fv_weight_rows'
 * bit for bit.  A weight of exactly 0 flags its sample: G is exactly 0 there, nothing is added anywhere and neither the
 * parts nor V are used (NaN or Inf there do not propagate).  A weight that is negative or not finite fails the call
 * with FV_ERR_ARG and fv_residual_chi2's message after it ran.  tpol not in {1, 4}, an antenna index outside [0, nant), a
 * null gains, nparts outside 0 .. 4, nparts = 0 without d_gains, a null part, d_gains or hgains without vis and a null
 * q_rows fail with FV_ERR_ARG before anything runs.  Host pointers. */
int fv_gain_weight_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, const void *gains, const void *d_gains, int nparts, const void *const *parts, void *vis,
                        const void *weights, double *q_rows, void *hgains);
/* fv_jones_weight_rows: fv_gain_weight_rows with one 2 x 2 complex (Jones) matrix per antenna and a direction of such
 * matrices (the kernel pair fv_sim_jones_weight_block queues): the weighting step of a Gauss-Newton product of
 * fv_jones_residual_chi2's chi2.  The rows (tpol = 4: 4 nbls values, V[x, y] at pol = 2 x + y), the pairs and jones are
 * fv_jones_residual_chi2's; d_jones: the direction dGamma in jones' layout (nrows, 2, 2, nant), or NULL; parts:
 * nparts = 0 .. 4 blocks as for fv_weight_rows (nparts = 0, the matrices-only direction, needs d_jones); vis: the forward V
 * at the real parameters, needed with d_jones or hjones, else it may be NULL.  Per baseline k = (a1, a2), with
 * G1 = Gamma[a1], G2 = Gamma[a2], H1 = dGamma[a1], H2 = dGamma[a2], U = ((P_0 + P_1) + P_2) + P_3 (0 for nparts = 0) and
 * S(X; A, B)[x, y] = sum_{x', y'} conj(A[y', y]) B[x', x] X[x', y'] formed as fv_jones_residual_chi2 forms V' = S(V; G1, G2)
 * (X conj(A) first, then B^T times it), in `precision`, every operation rounded on its own, in this order:
 *   U' = (S(U; G1, G2) + S(V; H1, G2)) + S(V; G1, H2)    (the first term alone without a direction; the tangent of V')
 *   G'[x, y] = 2 (w[x, y] U'[x, y])                       quad row += w |U'|^2  (terms formed and added in fp64)
 *   stored G[x', y'] = sum_{x, y} conj(G2[x', x]) G'[x, y] G1[y', y]   (what the public sky adjoints read)
 *   hjones[a, y', y] += sum_x conj(G'[x, y]) (G2^T V)[x, y']        for every k with a1[k] = a
 *   hjones[a, x', x] += sum_y G'[x, y] conj((V conj G1)[x', y])     for every k with a2[k] = a
 * G is written in place into parts[0], or into vis for nparts = 0 (everything else is read only); q_rows[i] is row i's
 * sum, reduced as fv_jones_residual_chi2 reduces; over all rows <p, H p> = 2 sum q_rows, the matrices' inner product being
 * Re sum conj(dGamma) hjones.  hjones: (nrows, 2, 2, nant) complex128, the matrices' block of H p in the convention of
 * gjones, or NULL (its kernel does not run); every term is formed in fp64 from the inputs of `precision` and added as
 * fv_jones_residual_chi2 adds gjones -- no floating-point atomics, the same input gives the same bits; an antenna without
 * a baseline gets exactly 0.  With identity matrices and no direction G and q_rows are fv_weight_rows' bit for bit.  A
 * weight of exactly 0 flags that one (x, y) sample: G' is exactly 0 there and nothing is added, while the baseline's other
 * samples still use all four values of U and V; a baseline with all four samples flagged stores G = 0 exactly and neither
 * its parts nor V are used (NaN or Inf there do not propagate).  A weight that is negative or not finite fails the call
 * with FV_ERR_ARG and fv_residual_chi2's message after it ran.  An antenna index outside [0, nant), a null jones, nparts
 * outside 0 .. 4, nparts = 0 without d_jones, a null part, d_jones or hjones without vis and a null q_rows fail with
 * FV_ERR_ARG before anything runs.  Host pointers. */
int fv_jones_weight_rows(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                         const void *jones, const void *d_jones, int nparts, const void *const *parts, void *vis,
                         const void *weights, double *q_rows, void *hjones);
int fv_inplace_rot(int device, int precision, const double *rot, void *b, int64_t n);
/* fv_astrom_topo: one time step of the device-side coordinate manager (see fv_sim_set_astrom): eq (3, n) ICRS unit
 * vectors -> topo (3, n) topocentric (east, north, up) unit vectors under one 31-double context -- what matvis'
 * CoordinateRotationERFA.rotate(t) leaves in all_coords_topo (cpu_simulate.py:937).                      */
int fv_astrom_topo(int device, int precision, const double *astrom, int64_t n, const void *eq, void *topo);

/* ---- fused simulator (the hot loop) ---------------------------------------------------------
 * One handle = one GPU context: streams, FFT twiddle / deconvolution tables, device-resident catalog / baselines /
 * beams / scratch.  A handle is not thread-safe; different handles are independent.
 * Replaces: GPUSimulationEngine._evaluate_vis_chunk stub (src/fftvis/gpu/gpu_simulate.py:62-91),
 * i.e. the GPU twin of CPUSimulationEngine._evaluate_vis_chunk
 * (src/fftvis/cpu/cpu_simulate.py:856-1071) and the helpers it calls
 * (_compute_apparent_coherency :90-202, _run_nufft :205-300, cpu/beams.py:129-246,
 *  cpu/utils.py:5-24).                                                                        */
typedef struct fv_sim fv_sim;

/* precision 1|2; eps: NUFFT accuracy (core/simulate.py:16-19 defaults are the caller's job);
 * upsampfac 2.0|1.25 (cpu/nufft.py:19 "upsample_factor", handed to finufft as is), or 0 = let every
 * fv_sim_run pick: 1.25 when eps >= 1e-8 (fp32: 1e-4; ten times that in 3-D), the fine grid at sigma = 2 has >= 4e6 cells
 * and >= 30 cells per source and target (200 in 3-D), else 2 -- the accuracy contract is eps either way;
 * polarized: nfeeds = 2 (cpu_simulate.py:589). */
int fv_sim_create(fv_sim **h, int device, int precision, double eps, double upsampfac,
                  int polarized);
int fv_sim_destroy(fv_sim *h);

/* Source catalog.  eq: (3, nsrc) equatorial unit vectors (x = cos dec cos ra, ...), real.
 * flux: coherency as prepared by prepare_source_catalog (cpu/utils.py:26-80), already x0.5:
 *   polarized_sky = 0: (nsrc, nfreq) real;  = 1: (nsrc, nfreq, 2, 2) complex.
 * on_device != 0: pointers are device pointers on this handle's GPU (e.g. tensors received by
 * an RCCL broadcast); the library copies either way and the caller keeps ownership.          */
int fv_sim_set_sources(fv_sim *h, int64_t nsrc, int nfreq, const void *eq, const void *flux,
                       int polarized_sky, int on_device);

/* Per-time equatorial -> topocentric ENU rotation matrices, (ntimes, 3, 3) float64 row-major:
 * the device-side stand-in for matvis CoordinateRotation.rotate/select_chunk as used at
 * cpu_simulate.py:937-946 (above-horizon selection up > 0 happens on the device).            */
int fv_sim_set_times(fv_sim *h, int ntimes, const double *rot_eq2enu);

/* Alternative to fv_sim_set_times for callers that own an astrometry engine (matvis
 * CoordinateRotationERFA/Astropy): per-time topocentric ENU unit vectors of EVERY catalog source,
 * (ntimes, 3, nsrc) real of the handle's precision -- what coord_mgr.rotate(ti) produces at
 * cpu_simulate.py:937 before the horizon cut.  Call after fv_sim_set_sources.                 */
int fv_sim_set_topo(fv_sim *h, int ntimes, int64_t nsrc, const void *topo, int on_device);

/* The coordinate manager on the device (the matvis manager the CPU engine builds at
 * cpu_simulate.py:693-709 and rotates per time at :937): instead of per-source vectors the caller hands over the
 * SOURCE-INDEPENDENT context of each time, astrom (ntimes, 31) float64 = one eraASTROM per time in ERFA's field order
 *   pmt, eb[3], eh[3] (Sun -> observer unit vector), em (au), v[3] (observer barycentric velocity / c), bm1,
 *   bpn[3][3] (row-major), along, phi, xpl, ypl, sphi, cphi, diurab, eral, refa, refb
 * -- what erfa.apco13 / astropy's erfa_astrom.apco fills in microseconds -- and the library applies it to every
 * catalog source in front of the horizon cut: light deflection by the Sun, annual aberration, bias-precession-
 * nutation, Earth rotation angle + longitude (eral), polar motion, diurnal aberration, rotation to the horizon,
 * refraction (refa = refb = 0: none) -- the published eraAtciqz / eraAtioq algorithms.  No (ntimes, 3, nsrc)
 * host stream (1.4 GB per 60 times at 1e6 sources).  A context with bpn = identity, v = 0, em huge, xpl = ypl =
 * diurab = refa = refb = 0 and eral = local sidereal angle is exactly fv_sim_set_times' rotation.
 * Replaces fv_sim_set_times / fv_sim_set_topo.  Parity versus ERFA itself is unpinned in this pipeline.    */
int fv_sim_set_astrom(fv_sim *h, int ntimes, const double *astrom);

/* Frequencies (Hz), float64 (nfreq). (cpu_simulate.py:969-973) */
int fv_sim_set_freqs(fv_sim *h, int nfreq, const double *freqs);

/* Array: rotation_matrix (3,3) float64 applied to topo before the NUFFT (cpu_simulate.py:961-962),
 * bls (3, nbls) float64 in SECONDS = R (a2 - a1) / c (cpu_simulate.py:650-659), is_coplanar
 * (cpu_simulate.py:655).                                                                      */
int fv_sim_set_array(fv_sim *h, const double *rotation_matrix, int64_t nbls, const double *bls,
                     int is_coplanar);

/* Lattice ("gridded") array: the type-1 path the reference takes by default for flat arrays whose
 * antennas sit on a lattice (cpu_simulate.py:634-637, 661-681; cpu_nufft2d_type1,
 * cpu/nufft.py:120-175).  basis_matrix (3,3) float64 in SECONDS (= lattice basis / (factor c),
 * :676) -- topo is rotated by its transpose (:964-965); bls_int (2, nbls) int32 lattice
 * coordinates of each baseline (:666-670); n_modes = 2 max|bls_int| + 1 (:673).  Alternative to
 * fv_sim_set_array; results equal the type-3 path's to the NUFFT accuracy.                     */
int fv_sim_set_array_type1(fv_sim *h, const double *basis_matrix, int64_t nbls, const int *bls_int,
                           int n_modes);

/* Beams (evaluate_beam, cpu/beams.py:12-89).  kind 0: analytic Airy dish, param[0] = diameter
 * [m]; E-field 2 J1(x)/x in all four Jones slots, power beam = its square.
 * kind 1: tabulated on a regular (za, az) grid; table is
 *   polarized:   (nfreq_tab, 2, 2, nza, naz) complex128  [ax, feed]
 *   unpolarized: (nfreq_tab, nza, naz) float64 power
 * with az periodic over 2 pi, za in [0, za_max] inclusive; nfreq_tab is 1 or nfreq.
 * order = beam_spline_opts["order"] (cpu/beams.py:69-74 -> pyuvdata az_za_map_coordinates ->
 * scipy.ndimage.map_coordinates): 0 = nearest node; 1 = bilinear; 2 .. 5 = interpolating B-spline of that
 * degree (the table is turned into spline coefficients on the device at upload; periodic in az,
 * mirrored in za).  1 and 3 have unrolled kernels, the others share one general path.
 * One order per handle.                                                                       */
int fv_sim_set_nbeams(fv_sim *h, int nbeams);
int fv_sim_set_beam_airy(fv_sim *h, int beam, double diameter);
/* The same dish with a complex factor per Jones slot, A[ax][feed] = jones_scale[ax][feed] 2 J1(x)/x
 * (jones_scale: 4 complex128 = 8 float64, row-major [ax][feed]; NULL = all ones), and a real factor on
 * the power beam, power_scale (2 J1(x)/x)^2.  How a third-party analytic Airy object is put on the device
 * in closed form: the host probes the object's own compute_response (cpu/beams.py:69-81 calls it per
 * slice), fits these factors and uses this entry only when every probe agrees to 1e-12 (e.g. pyuvdata's
 * AiryBeam: 1/sqrt(2) in every slot); otherwise the object is sampled onto a table.               */
int fv_sim_set_beam_airy_scaled(fv_sim *h, int beam, double diameter, const double *jones_scale,
                                double power_scale);
int fv_sim_set_beam_table(fv_sim *h, int beam, int nfreq_tab, int nza, int naz, double za_max,
                          const void *table, int order);

/* Beam pairs (prepare_beam_evaluation, cpu/beams.py:91-127): for pair p, beams (bi[p], bj[p]),
 * baseline indices idx[off[p] .. off[p+1]) and their `flipped` flags.  npairs = 1, bi=bj=0,
 * idx = 0..nbls-1, no flips is the beam_idx=None case.                                        */
int fv_sim_set_beam_pairs(fv_sim *h, int npairs, const int *bi, const int *bj, const int64_t *off,
                          const int *idx, const signed char *flipped);

/* Eigenbeam ("basis") mode, _compute_basis_visibilities (cpu_simulate.py:303-470): the handle's
 * beams 0..nbasis-1 are the K basis beams (E-field; polarized engine only, wrapper.py:280-283);
 * coefs is beam_coefs (nant, nbasis, nfreq) complex of the handle's precision; ant1/ant2 (nbls)
 * give each baseline's antenna indices into coefs (:920-921).  Replaces any beam pairs: every
 * (k <= l) term runs over all baselines without flips (:402-404) and is contracted as
 * conj(c[a1,k]) c[a2,l] V_kl + [l != k] conj(c[a1,l]) c[a2,k] V_kl^T (:461-468).
 * Call after fv_sim_set_array, fv_sim_set_freqs and the beams.                                */
int fv_sim_set_basis(fv_sim *h, int nant, int nbasis, int nfreq, const void *coefs, const int *ant1,
                     const int *ant2);

/* Two places where the reference's arithmetic differs from the exact symmetry of the visibilities (SURVEY
 * App. B Q1 / Q2).  on != 0 (the default): as the reference -- (1) a flipped baseline of a two-beam polarized pair
 * is evaluated at -b and conjugated, its 2 x 2 feed block NOT transposed (cpu_simulate.py:271,298); (2) the
 * eigenbeam (l, k) term reuses V_kl(b) transposed (:464-468), exact for real-valued basis beams only.
 * on == 0: (1) V_ji(b) = V_ij(-b)^H, conjugated and transposed; (2) V_lk(b) = conj(V_kl(-b))^T -- one more
 * gather at -b per off-diagonal term of complex basis beams.  Sticky on the handle; takes effect at the next run. */
int fv_sim_set_reference_compat(fv_sim *h, int on);

/* Source-axis chunking: the `for chunk in range(nchunks)` loop inside the reference's time loop
 * (cpu_simulate.py:939-946; visibilities accumulate with += over chunks, :1024,1069) and matvis'
 * source_buffer (cpu_simulate.py:693-704: the above-horizon arrays of a chunk hold
 * source_buffer x chunk size sources).  Every time step then processes the catalog in nchunks
 * consecutive pieces whose per-time device scratch (coordinates, bin sort, kernel weights, strengths)
 * is sized by one piece; the catalog itself stays resident.  A chunk with more sources above the
 * horizon than source_buffer allows fails the run (FV_ERR_ARG at the next synchronisation), as matvis
 * raises.  Defaults: nchunks = 1, source_buffer = 1.                                           */
int fv_sim_set_chunking(fv_sim *h, int nchunks, double source_buffer);

/* Run times [t0, t1) x freqs [f0, f1).  Result layout is the reference's FINAL layout
 * (cpu_simulate.py:850-854): polarized (nf_here, nt_here, 2, 2, nbls), else (nf_here, nt_here,
 * nbls), complex of the handle's precision.  out_on_device = 0: `out` is a host buffer (the
 * call synchronises); != 0: `out` is a device buffer and the call only enqueues work on the
 * handle's stream -- use fv_sim_sync().  A device `out` must be ordinary (coarse-grained) hipMalloc
 * memory on the handle's GPU: small 2-D grids are gathered with fp64 atomics compiled with
 * -munsafe-fp-atomics, which fine-grained or managed memory does not honour.
 * Bad input met on the device (source vectors that are NaN or not unit length, so that they fall
 * outside the planned grid; a type-1 entry overflow) fails the run at the next host
 * synchronisation -- this call for a host `out`, fv_sim_sync() otherwise -- with FV_ERR_ARG /
 * FV_ERR_INTERNAL; the output of that run is invalid.                                          */
int fv_sim_run(fv_sim *h, int t0, int t1, int f0, int f1, void *out, int out_on_device);
/* The same into a block INSIDE a larger host array in the final layout: channel f of the block starts
 * f * out_f_stride elements after `out` (0: contiguous, = fv_sim_run with a host `out`); its times are contiguous.
 * This is the reference's `vis[tc][..., fc] = future` (src/fftvis/cpu/cpu_simulate.py:843-847) without the copy: the
 * time blocks of a run that does not fit the device, and the ranks of a sharded run, deliver straight into their
 * slice of the result -- pinned in place run by run and filled from a copy stream while later time steps compute.
 * shared != 0: other processes write the rest of the array (one result in shared memory for all ranks of a node): the
 * pinning helper then only reads the block's pages when it touches them and registers nothing beyond its runs.        */
int fv_sim_run_into(fv_sim *h, int t0, int t1, int f0, int f1, void *out, int64_t out_f_stride, int shared);
/* Adjoint of fv_sim_run with everything the fv_sim_set_* calls configured: gflux += A^T G for times [t0, t1) x freqs
 * [f0, f1), where A maps the catalog's fluxes to the visibilities fv_sim_run computes and A^T is taken for the real inner
 * products, Re <A F, G> = <F, A^T G> (flipped baselines are conjugated: the map is real-linear).  gvis: G, complex of
 * the handle's precision in fv_sim_run's output layout for that block.  gflux: (nsrc, nfreq) of the precision's real
 * type for a Stokes-I catalog, (nsrc, nfreq, 2, 2) complex for a coherency catalog (the gradient Gc with
 * Re <A C, G> = Re sum conj(Gc) C); only channels [f0, f1) receive a contribution.  accumulate = 0: gflux is zeroed
 * first.  The *_on_device flags as in fv_sim_run (device buffers must be complete when the call is made); the call
 * synchronises.  The bulk device memory it uses beyond what fv_sim_run holds (the grids of a second transform per
 * lane, fp64 accumulators of at most FFTVIS_HIP_ADJ_ACC_BYTES per lane -- channel blocks --, staged host buffers) is
 * given back when it exceeds FFTVIS_HIP_ADJ_KEEP_BYTES (default 256 MiB); the second transforms' tables and
 * per-baseline arrays stay with the handle.  Lattice
 * arrays use the type-3 transform here as well unless fv_sim_set_adjoint_path selects the type-2 transform (its planes
 * and entry records fall under the same give-back rule).  A handle with basis beams (fv_sim_set_basis) and NaN in G fail with
 * FV_ERR_ARG.  Sums run in fp64, per lane in a fixed order, so that a run is
 * bitwise reproducible for a given FFTVIS_HIP_LANES.                                                                   */
int fv_sim_run_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                       int gflux_on_device, int accumulate);
/* The same for a handle with basis beams (fv_sim_set_basis), plus the gradient with respect to the coefficients.
 * gflux += A^T G as above, A the basis-beam map from the catalog's fluxes to the visibilities (linear in the fluxes for
 * fixed coefficients C).  gcoefs += the gradient of the map's sesquilinear dependence on C: with dV[C; D] the derivative
 * of the visibilities along a complex direction D of the coefficients, Re <dV[C; D], G> = Re <D, gcoefs> for every D
 * (dL = Re sum conj(gcoefs) dC when G = dL/dV: what torch returns for a complex leaf).  gcoefs: (nant, nbasis, nfreq)
 * complex of the handle's precision, the layout of fv_sim_set_basis' coefs; only channels [f0, f1) receive a
 * contribution.  Either output may be NULL (not wanted, its pass does not run), not both.  accumulate = 0: the outputs
 * are zeroed first.  fv_sim_set_reference_compat selects the form of the (l, k) terms as in fv_sim_run.  The flux pass is
 * fv_sim_run_adjoint's with per-baseline coefficient weights; the coefficient pass is a forward run whose gather forms
 * the inner products of G with the basis visibilities in fp64 -- (nbasis^2, channels, nbls) complex per lane, at most
 * FFTVIS_HIP_ADJ_ACC_BYTES per lane (channel blocks) -- followed by a per-(antenna, basis index, channel) sum over the
 * antenna's baselines in a fixed order.  No atomics: bitwise reproducible for a given FFTVIS_HIP_LANES.  Memory is given
 * back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule above.  The call synchronises.  A handle without fv_sim_set_basis, both
 * outputs NULL, *_on_device flags other than 0 or 1 and NaN in G fail with FV_ERR_ARG.                                  */
int fv_sim_run_basis_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                             int gflux_on_device, void *gcoefs, int gcoefs_on_device, int accumulate);
/* Gradient of fv_sim_run's visibilities with respect to the baseline vectors, for times [t0, t1) x freqs [f0, f1).  Every
 * forward path evaluates, to the handle's tolerance, out_k = cj_k( sum_j c_j exp(i nu s_k b'_k . x_j) ) with b' = R b / c the
 * rotated baselines in seconds (src/fftvis/cpu/cpu_simulate.py:650-658, uvw = bls * freq at :972-973), x = 2 pi R topo
 * (:961-967) and s_k = -1, cj_k = conj for a flipped baseline (:298); the beams, the horizon cut and the strengths c do not
 * depend on the positions.  So d out_k / d b'_k,d = i nu D'_d, D'_d what fv_sim_run writes when every source's strengths
 * are multiplied by x_j,d -- for both fv_sim_set_reference_compat forms, flipped baselines and every packing --, and with
 * G = dL/dV, dL = Re sum conj(G) dV:
 *     gbls[k, d] += (R^T g'[k])_d / c,     g'[k, d] = - sum_{f, t, r} nu_f Im( conj(G[f, t, r, k]) D'_d[f, t, r, k] ).
 * gvis: G, complex of the handle's precision in fv_sim_run's output layout for that block.  gbls: (nbls, 3) float64 at
 * either precision, per metre, in the frame of the vectors b whose image R b / c fv_sim_set_array received (R, bls: its
 * inputs; R^T / c takes the gradient back); every listed baseline is an independent vector.  On a coplanar handle the
 * forward drops b'_z; the third component of g' is still formed (D'_z weights by the sources' height coordinate).
 * accumulate = 0: gbls is zeroed first.  The *_on_device flags as in fv_sim_run (device buffers must be complete when the
 * call is made); the call synchronises.  The pass is a forward run per channel block -- one strengths launch that writes
 * the three weighted sets, then per component spread, FFT and a gather that forms the inner products with G in fp64,
 * (3, channels, nbls) complex per lane, at most FFTVIS_HIP_ADJ_ACC_BYTES per lane -- followed by a per-baseline sum over
 * channels and lanes in a fixed order.  No atomics: bitwise reproducible for a given FFTVIS_HIP_LANES.  Memory is given
 * back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule of fv_sim_run_adjoint.  A lattice handle (fv_sim_set_array_type1: set the
 * array with fv_sim_set_array instead), a handle with basis beams (fv_sim_run_basis_position_adjoint is the pass there),
 * a null pointer, a flag other than 0 or 1 and NaN in G fail with FV_ERR_ARG.                                            */
int fv_sim_run_position_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gbls,
                                int gbls_on_device, int accumulate);
/* Gradient of fv_sim_run's visibilities with respect to the sources' directions, for times [t0, t1) x freqs [f0, f1).
 * Every forward path evaluates, to the handle's tolerance, out[f,t,r,k] = cj_k( sum_j c_jr(f,t; n_j(t)) exp(i nu_f s_k b'_k .
 * x_j(t)) ), x = 2 pi R n, n_j(t) the source's topocentric unit vector (east, north, up) at time t -- R_t eq, the vectors of
 * fv_sim_set_topo, or the astrometry context applied on the device -- and c the apparent strengths, which depend on n
 * through the beams.  With G = dL/dV, dL = Re sum conj(G) dV, and Z the transposed transform of fv_sim_run_adjoint,
 *     gtopo[t - t0, j, :] += P_n ( 2 pi R^T sum_f nu_f ( -Im sum_r c_jr Z(d)_jr )_d  +  sum_f grad_n Re sum_r c_jr(n) Z_jr ),
 * Z(d) the same transform of the strengths times the d-th coordinate of the run's sign-adjusted baseline vector (the phase
 * term), the second sum the beams' own dependence on the direction with Z held fixed, by central differences along two
 * tangent great circles at a fixed angular step (the beam term), and P_n = 1 - n n^T: n is a unit vector, so only the
 * tangential gradient is defined, dL = sum_{t,j} gtopo[t,j] . delta_j(t) for every small displacement delta perpendicular
 * to n.  A source below the horizon at time t gets exactly 0 there (the cut is not differentiated).  It is the gradient of
 * the smooth exact map, whichever path the forward takes, for both fv_sim_set_reference_compat forms.
 * gvis: G, complex of the handle's precision in fv_sim_run's output layout for that block.  gtopo: (t1 - t0, nsrc, 3)
 * float64 at either precision.  accumulate = 0: gtopo is zeroed first.  The *_on_device flags as in fv_sim_run; the call
 * synchronises.  The fluxes are the forward's (fv_sim_set_sources).  The pass is fv_sim_run_adjoint's loop with 1 + D
 * transforms per (time, frequency group, beam pair), D = 2 on a coplanar handle and 3 otherwise, and five beam evaluations
 * per (source, channel); a lane's fp64 accumulator is (nsrc, channels of a block, 3), at most FFTVIS_HIP_ADJ_ACC_BYTES.  No
 * atomics, one lane per time step: bitwise reproducible whatever FFTVIS_HIP_LANES.  Memory is given back under the
 * FFTVIS_HIP_ADJ_KEEP_BYTES rule of fv_sim_run_adjoint.  FFTVIS_HIP_SRC_BEAM_STEP overrides the beam term's step (radians;
 * for measurements).  A lattice handle (fv_sim_set_array_type1: set the array with fv_sim_set_array instead), a handle with
 * basis beams, a null pointer, a flag other than 0 or 1 and NaN in G fail with FV_ERR_ARG.                              */
int fv_sim_run_source_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gtopo,
                              int gtopo_on_device, int accumulate);
/* Forward-mode tangent (Jacobian-vector product) of fv_sim_run's visibilities along a change of the baseline vectors
 * and / or of the sources' directions, for times [t0, t1) x freqs [f0, f1):
 *     out = dV = sum_k dV/db_k . dbls[k]  +  sum_{t,j} dV/dn_j(t) . P_n dtopo[t - t0, j],     P_n = 1 - n n^T.
 * With out_k = cj_k( sum_j c_j(n_j) exp(i nu s_k b'_k . x_j) ), b' = R b / c, x = 2 pi R n as above, both derivatives of
 * the exact map are forward transforms of other strengths:
 *     baselines:  dV[.., k] += sum_d i nu_f (R dbls[k] / c)_d D'_d[.., k],   D'_d the forward of the strengths times x_j,d,
 *     sources:    dV[.., k] += forward of dc_j  +  sum_d i nu_f b'_k,d (forward of c_j dx_j,d),     dx = 2 pi R P_n dtopo,
 * dc_j = |delta| (c(n+) - c(n-)) / 2h the beams' change along the great circle through n towards delta = P_n dtopo, n+- =
 * cos(h) n +- sin(h) delta / |delta|, evaluated in fp64 (two displaced beam evaluations per source and channel; exactly 0
 * where delta = 0).  A flipped baseline conjugates -i nu b' X into +i nu b' conj(X): neither part has a sign case.  It is
 * the tangent of the smooth exact map, whichever path the forward takes, for both fv_sim_set_reference_compat forms, and
 * the transpose of the two gradients above:  Re <dV, G> = sum dbls . gbls + sum dtopo . gtopo  for EVERY input (P_n removes
 * the radial part of dtopo), with gbls and gtopo those of fv_sim_run_position_adjoint and fv_sim_run_source_adjoint.
 * out: complex of the handle's precision in fv_sim_run's layout for that block, always overwritten (no accumulate flag).
 * dbls: (nbls, 3) float64 in metres, in the frame of the vectors b whose image R b / c fv_sim_set_array received (the frame
 * gbls comes back in); every listed baseline is an independent vector.  dtopo: (t1 - t0, nsrc, 3) float64, ENU.  Either
 * input may be NULL -- its rounds do not run --, not both.  A source below the horizon at time t contributes exactly 0
 * there and its dtopo row is not read (the cut is not differentiated).  On a coplanar handle the up component of dbls
 * still enters (D'_z weights by the sources' height coordinate), and the source side runs D = 2 sets, since b'_z = 0.
 * The *_on_device flags as in fv_sim_run (device buffers must be complete when the call is made); the call synchronises.
 * The pass is a forward run per channel block: per (time, source chunk, frequency group, beam pair, height term) one
 * strengths launch per input, then 3 and / or 1 + D rounds of spread, FFT and a gather that ADDS i nu_f w V (or V, the
 * beam term) into the zeroed output block, one owner thread per slot.  No atomics, one lane per time step: bitwise
 * reproducible for a given FFTVIS_HIP_LANES.  A host destination receives the block in one copy at the end.  Memory is
 * given back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule of fv_sim_run_adjoint.  FFTVIS_HIP_SRC_BEAM_STEP overrides the step
 * h (radians; for measurements).  A lattice handle (fv_sim_set_array_type1), a handle with basis beams
 * (fv_sim_run_basis_position_tangent serves dbls there), a null handle, a
 * null out, both inputs NULL, a flag other than 0 or 1 and a value in either input that is not finite (detected before
 * anything runs; the handle stays usable) fail with FV_ERR_ARG.                                                          */
int fv_sim_run_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device, const double *dtopo,
                       int dtopo_on_device, void *out, int out_on_device);
/* Forward-mode tangent of a basis-beam handle's visibilities (fv_sim_set_basis) along ndir directions of the coefficients,
 * for times [t0, t1) x freqs [f0, f1).  With V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b), M_kl the visibilities of basis
 * beams k and l, the derivative along a complex direction D of the coefficients is
 *     dV_b[C; D] = sum_kl ( conj(D[a1,k]) C[a2,l] + conj(C[a1,k]) D[a2,l] ) M_kl(b),
 * real-linear in D, and M_kl depends on neither C nor D: out[q] = dV[C; D_q] is ONE forward run whose gathers carry the
 * differentiated weights, and the ndir directions share every transform.  It is the transpose of
 * fv_sim_run_basis_adjoint's coefficient gradient, Re <dV[C; D], G> = Re <D, gcoefs>, and dV[C; D] = (V(C + D) - V(C - D)) / 2
 * exactly (the map is sesquilinear).  fv_sim_set_reference_compat selects the form of the (l, k) terms as in fv_sim_run.
 * dcoefs: (ndir, nant, nbasis, nfreq) complex of the handle's precision, every direction laid out like fv_sim_set_basis'
 * coefs; only channels [f0, f1) are read.  out: (ndir, f1 - f0, t1 - t0, 2, 2, nbls) complex of the handle's precision,
 * every direction in fv_sim_run's layout for that block, always overwritten (no accumulate flag).  The *_on_device flags as
 * in fv_sim_run (device buffers must be complete when the call is made); the call synchronises.  The weights are summed
 * in fp64 before the product with M_kl, so directions whose two halves cancel (D = i C) give rounding-level output.  One
 * owner thread per slot and launch, a time step's slots written by its own lane only: no atomics, bitwise reproducible
 * for a given FFTVIS_HIP_LANES, and a direction's output does not depend on the others in the call.  A host destination
 * receives the output in one copy at the end.  The staged directions and output are given back under the
 * FFTVIS_HIP_ADJ_KEEP_BYTES rule of fv_sim_run_adjoint.  A handle without fv_sim_set_basis, a null handle, a null out, a
 * null dcoefs, ndir < 1, a flag other than 0 or 1 and an entry of dcoefs that is not finite (detected before anything runs;
 * the handle stays usable) fail with FV_ERR_ARG.                                                                          */
int fv_sim_run_basis_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const void *dcoefs, int dcoefs_on_device, int ndir,
                             void *out, int out_on_device);
/* Gradient of a basis-beam handle's visibilities (fv_sim_set_basis) with respect to the baseline vectors, for times
 * [t0, t1) x freqs [f0, f1): fv_sim_run_position_adjoint's quantity for V_b = sum_kl conj(C[a1,k]) C[a2,l] M_kl(b).
 * Every M_kl is a sum over sources of strengths that do not depend on the positions times exp(i nu s_b b' . x_j), so
 *     dV_b / db'_d = i nu D'_d(b),   D'_d the basis forward of the strengths times x_j,d,
 *     gbls[k, d] += - sum_{f, t, r} (2 pi nu_f / c) Im( conj(G) D_d ).
 * gvis, gbls, the flags and accumulate as in fv_sim_run_position_adjoint: gbls is (nbls, 3) float64 per metre in the
 * frame of the vectors given to fv_sim_set_array, and the third component is also returned on a coplanar handle.  The
 * pass is the basis forward run per channel block -- every (k <= l) term, fv_sim_set_reference_compat's two forms of the
 * (l, k) term, source chunks, lanes, height terms -- with three strength sets per launch and three transforms per term;
 * the gather applies the basis weights in fp64 and every term adds into ONE (3, channels of the block, nbls) complex fp64
 * buffer per stream (it does not grow with the number of basis beams), cut into channel blocks under
 * FFTVIS_HIP_ADJ_ACC_BYTES.  One owner thread per slot and launch, buffers summed in lane order: no atomics, bitwise
 * reproducible for a given FFTVIS_HIP_LANES.  Memory is given back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule of
 * fv_sim_run_adjoint.  Not covered: lattice handles.  A handle without
 * fv_sim_set_basis (fv_sim_run_position_adjoint is the pass there), a lattice handle, a null handle, a null gvis or gbls,
 * a flag other than 0 or 1 and NaN in gvis (detected before anything runs; the handle stays usable) fail with
 * FV_ERR_ARG.                                                                                                            */
int fv_sim_run_basis_position_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device,
                                      double *gbls, int gbls_on_device, int accumulate);
/* Forward-mode tangent of a basis-beam handle's visibilities along a direction of the baseline vectors, the transpose of
 * fv_sim_run_basis_position_adjoint:  out[.., k] = sum_d i (2 pi nu_f / c) dbls[k, d] D_d[.., k],  Re <out, G> = sum
 * dbls . gbls.  dbls: (nbls, 3) float64 in metres, in the frame of fv_sim_set_array's vectors.  out: fv_sim_run's layout
 * for the block, complex of the handle's precision, always overwritten.  The pass is that of the adjoint, the gather
 * adding i nu w (w1 V, w2 V) with the basis weights formed in fp64 into the zeroed block; a time step's slots are written
 * by its own lane only: bitwise reproducible for a given FFTVIS_HIP_LANES.  Channel blocks and memory as in
 * fv_sim_run_tangent.  A handle without fv_sim_set_basis (fv_sim_run_tangent is the pass there), a lattice handle, a null
 * handle, a null out or dbls, a flag other than 0 or 1 and a value of dbls that is not finite (detected before anything
 * runs; the handle stays usable) fail with FV_ERR_ARG.                                                                    */
int fv_sim_run_basis_position_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device,
                                      void *out, int out_on_device);
/* Gradient of a basis-beam handle's visibilities (fv_sim_set_basis) with respect to the sources' directions, for times
 * [t0, t1) x freqs [f0, f1): fv_sim_run_source_adjoint's quantity for V_b = sum_{k<=l} (w1 M_kl(b) at slot r + w2 M_kl(b)
 * at the feed-transposed slot), w1 = conj(C[a1,k]) C[a2,l], w2 = conj(C[a1,l]) C[a2,k]; with fv_sim_set_reference_compat
 * off the (l, k) part of an off-diagonal term is conj(M_kl(-b))^T.  Every M_kl is a sum over sources of the strengths
 * c^{kl}(n_j) of basis beams k and l times exp(i nu b' . x_j), so per term the gradient is that of the source pass:
 *     gtopo[t - t0, j, :] += P_n sum_terms ( 2 pi R^T sum_f nu_f ( -Im sum_r c^{kl}_jr Z(d)_jr )_d
 *                                            +  sum_f grad_n Re sum_r c^{kl}_jr(n) Z_jr ),
 * Z the transposed transform of the term's weighted strengths as fv_sim_run_basis_adjoint's flux pass forms them (in the
 * exact form with a mirrored half at -b, whose moments take the coordinates -b), Z(d) that of the strengths times the d-th
 * coordinate.  Tangential, exactly 0 below the horizon, the cut not differentiated; the beam term is 0 by definition
 * between two order-0 tables, decided per term.  gvis, gtopo, the flags and accumulate as in fv_sim_run_source_adjoint.
 * The pass is that one's loop over the (k <= l) terms: 1 + D transforms and five beam evaluations per (term, time,
 * frequency group), every term adding into the lane's (nsrc, channels of a block, 3) fp64 accumulator in stream order,
 * one reduction per time step.  No atomics: bitwise reproducible whatever FFTVIS_HIP_LANES.  Channel blocks
 * (FFTVIS_HIP_ADJ_ACC_BYTES), source chunks, lanes and the FFTVIS_HIP_ADJ_KEEP_BYTES rule as there.  Not covered: lattice
 * handles.  A handle without fv_sim_set_basis (fv_sim_run_source_adjoint is the pass there), a lattice handle, a null
 * handle, a null gvis or gtopo, a flag other than 0 or 1 and NaN in gvis (detected before anything runs; the handle stays
 * usable) fail with FV_ERR_ARG.                                                                                          */
int fv_sim_run_basis_source_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device,
                                    double *gtopo, int gtopo_on_device, int accumulate);
/* Joint sky adjoint: fv_sim_run_adjoint's flux gradient AND fv_sim_run_source_adjoint's direction gradient of the same G in
 * one pass, for times [t0, t1) x freqs [f0, f1) -- what a fit of the sources' fluxes and positions together needs per
 * step.  The source pass's first transform per (time, frequency group, beam pair) is the flux adjoint's Z -- the same
 * strengths, plan and targets --, so the 1 + D transforms of that pass serve both: after them Z is contracted with the
 * beams exactly as fv_sim_run_adjoint does (its kernel on the same values) into a flux accumulator per lane, summed in lane
 * order into gflux after each channel block, and gtopo comes from the source pass's own kernels unchanged.  gflux: the
 * shape and type fv_sim_run_adjoint documents, only channels [f0, f1) receive a contribution.  gtopo: (t1 - t0, nsrc, 3)
 * float64 as in fv_sim_run_source_adjoint.  accumulate = 0: both outputs are zeroed first; 1: both are added to.  The
 * *_on_device flags per buffer as in fv_sim_run; the call synchronises once, at its end.  A lane's fp64 accumulators take
 * 24 + 8 comps bytes per (source, channel of a block), comps = 1 for Stokes-I catalogs and 8 for coherency catalogs, at
 * most FFTVIS_HIP_ADJ_ACC_BYTES (channel blocks).  No atomics, fixed orders: bitwise reproducible for a given
 * FFTVIS_HIP_LANES, and gtopo whatever it is.  Memory is given back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule of
 * fv_sim_run_adjoint.  A lattice handle (fv_sim_set_array_type1: set the array with fv_sim_set_array instead), a handle
 * with basis beams (fv_sim_run_basis_sky_adjoint is the pass there), a null handle, a null gvis, gflux or gtopo, a flag
 * other than 0 or 1 and NaN in gvis (detected before anything runs; the handle stays usable) fail with FV_ERR_ARG.         */
int fv_sim_run_sky_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                           int gflux_on_device, double *gtopo, int gtopo_on_device, int accumulate);
/* The same for a handle with basis beams (fv_sim_set_basis): fv_sim_run_basis_adjoint's gflux and
 * fv_sim_run_basis_source_adjoint's gtopo from that pass's 1 + D transforms per (k <= l) term, one transform per term
 * fewer than the two calls.  The term's Z is contracted with its pair of basis beams as in fv_sim_run_basis_adjoint's flux
 * pass; fv_sim_set_reference_compat selects the form of the (l, k) terms as in fv_sim_run.  Arguments, accumulators, channel
 * blocks and memory as in fv_sim_run_sky_adjoint.  The coefficients' gradient is fv_sim_run_basis_adjoint's (its transforms
 * run the other way).  A handle without fv_sim_set_basis (fv_sim_run_sky_adjoint is the pass there), a lattice handle, a
 * null handle, a null gvis, gflux or gtopo, a flag other than 0 or 1 and NaN in gvis (detected before anything runs; the
 * handle stays usable) fail with FV_ERR_ARG.                                                                              */
int fv_sim_run_basis_sky_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                                 int gflux_on_device, double *gtopo, int gtopo_on_device, int accumulate);
/* Forward-mode tangent of a basis-beam handle's visibilities along a change of the sources' directions, the transpose of
 * fv_sim_run_basis_source_adjoint:  out = sum_{t,j} dV/dn_j(t) . P_n dtopo[t - t0, j],  Re <out, G> = sum dtopo . gtopo.
 * dtopo: (t1 - t0, nsrc, 3) float64, ENU; a row of a source below the horizon is not read.  out: fv_sim_run's layout for
 * the block, complex of the handle's precision, always overwritten.  The pass is the basis forward run per channel block:
 * per (k <= l) term the 1 + D strength sets of fv_sim_run_tangent with the term's beams, and 1 + D rounds of spread, FFT
 * and a gather that adds i nu_f b'_d (w1 V, w2 V) with the basis weights formed in fp64 -- (w1 V, w2 V) as they are in
 * the beam term's round -- into the zeroed block, for both forms of the (l, k) term; a time step's slots are written by
 * its own lane only: bitwise reproducible for a given FFTVIS_HIP_LANES.  Channel blocks and memory as in
 * fv_sim_run_tangent.  A handle without fv_sim_set_basis (fv_sim_run_tangent is the pass there), a lattice handle, a null
 * handle, a null out or dtopo, a flag other than 0 or 1 and a value of dtopo that is not finite (detected before anything
 * runs; the handle stays usable) fail with FV_ERR_ARG.                                                                    */
int fv_sim_run_basis_source_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dtopo, int dtopo_on_device,
                                    void *out, int out_on_device);
/* Fit objective of the block times [t0, t1) x freqs [f0, f1):  gvis = G = 2 w (V - data) = d chi2 / dV  and
 * chi2_ft[(f - f0) (t1 - t0) + (t - t0)] = sum over the (time, frequency) row of w |V - data|^2,  V what fv_sim_run
 * computes for the block -- which never leaves the device.  The call is fv_sim_run into gvis (a device buffer, or for a
 * host destination the handle's staged block, copied back once at the end as fv_sim_run_tangent does), then the two
 * kernels of fv_residual_chi2 on the handle's main stream behind the joined lanes, then one synchronisation that brings
 * chi2_ft, (f1 - f0) (t1 - t0) HOST doubles.  data: fv_sim_run's layout for the block, complex of the handle's
 * precision; weights: the same shape, real of that precision, or NULL (every weight 1); inverse variances, 0 flags a
 * sample with fv_residual_chi2's rules (G exactly 0, the datum not used).  gvis is what every fv_sim_run_*_adjoint of
 * this handle takes as its input.  The *_on_device flags as in fv_sim_run (device buffers must be complete when the call
 * is made); host data and weights are staged on the device, and their bytes are given back under the
 * FFTVIS_HIP_ADJ_KEEP_BYTES rule of fv_sim_run_adjoint.  Works on every handle fv_sim_run works on: lattice handles (the
 * type-1 forward), basis beams, source chunks, height terms.  The rows' sums are bitwise reproducible for a given
 * forward result.  A null handle, a null data, gvis or chi2_ft, a flag other than 0 or 1 and an empty range fail with
 * FV_ERR_ARG before anything runs; a weight that is negative or not finite, or a datum that is not finite at a positive
 * weight, fails the call with FV_ERR_ARG after it ran (counted by the residual kernel itself: no extra pass over data and
 * weights): gvis and chi2_ft are then invalid and the handle stays usable.                                                */
int fv_sim_run_residual(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device, const void *weights,
                        int weights_on_device, void *gvis, int gvis_on_device, double *chi2_ft);
/* The antenna pair (ant1[k], ant2[k]) of every baseline of the configured array, indices into the nant rows of the gains
 * fv_sim_run_residual_gains takes: uploaded once, with the per-antenna incidence lists its gain gradient walks.  Call
 * it after fv_sim_set_array / fv_sim_set_array_type1; setting other baselines invalidates it.  An index outside
 * [0, nant) fails with FV_ERR_ARG.                                                                                        */
int fv_sim_set_gain_pairs(fv_sim *h, int nant, const int *ant1, const int *ant2);
/* fv_sim_run_residual with per-antenna gains: the data model is V' = conj(g[ant1]) g[ant2] V.  The call is
 * fv_sim_run_residual's -- forward into gvis, kernels on the main stream, one synchronisation -- with the two kernels of
 * fv_gain_residual_chi2: gvis = G = d chi2 / dV (NOT 2 w (V' - data): the gain product's transpose is applied), chi2_ft
 * the rows of sum w |V' - data|^2.  gains: (f1 - f0, t1 - t0, nfeed, nant) complex of the handle's precision; ggains: the
 * same shape in complex128, the gradient with respect to the gains (d chi2 = Re sum conj(ggains) dg), or NULL.  Host gains
 * are staged and given back with host data and weights under the FFTVIS_HIP_ADJ_KEEP_BYTES rule.  A null handle, a null
 * data, gains, gvis or chi2_ft, a flag other than 0 or 1, an empty range and missing pairs fail with FV_ERR_ARG before
 * anything runs; bad weights and data as for fv_sim_run_residual.                                                        */
int fv_sim_run_residual_gains(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device,
                              const void *weights, int weights_on_device, const void *gains, int gains_on_device, void *gvis,
                              int gvis_on_device, double *chi2_ft, void *ggains, int ggains_on_device);
/* fv_sim_run_residual with one 2 x 2 complex (Jones) matrix per antenna: the data model is fv_jones_residual_chi2's
 * V' = G2^T V conj(G1) on the [x, y] block of every baseline.  The call is fv_sim_run_residual_gains' -- forward into gvis,
 * kernels on the main stream, one synchronisation -- with the kernels of fv_jones_residual_chi2: gvis = G = d chi2 / dV,
 * chi2_ft the rows of sum w |V' - data|^2.  jones: (f1 - f0, t1 - t0, 2, 2, nant) complex of the handle's precision;
 * gjones: the same shape in complex128, the gradient with respect to the matrices (d chi2 = Re sum conj(gjones) dGamma),
 * or NULL.  Needs fv_sim_set_gain_pairs and a polarized handle.  Host matrices are staged and given back with host data
 * and weights under the FFTVIS_HIP_ADJ_KEEP_BYTES rule, and so is the fp64 block of row terms the handle holds for the
 * call.  A null handle, a null data, jones, gvis or chi2_ft, a flag other than 0 or 1, an empty range, missing pairs and
 * a handle that is not polarized fail with FV_ERR_ARG before anything runs; bad weights and data as for
 * fv_sim_run_residual.                                                                                                    */
int fv_sim_run_residual_jones(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device,
                              const void *weights, int weights_on_device, const void *jones, int jones_on_device, void *gvis,
                              int gvis_on_device, double *chi2_ft, void *gjones, int gjones_on_device);
/* Gauss-Newton product of the block times [t0, t1) x freqs [f0, f1): the tangent U = J p arrives as nparts = 1 .. 4 DEVICE
 * blocks parts_dev[j] in fv_sim_run's layout for the block, complex of the handle's precision -- what fv_sim_run and the
 * fv_sim_run_*_tangent calls of this handle wrote with out_on_device = 1 -- and the two kernels of fv_weight_rows on the
 * handle's main stream leave  G = 2 w U  in parts_dev[0]  and
 * q_ft[(f - f0) (t1 - t0) + (t - t0)] = sum over the (time, frequency) row of w |U|^2,  (f1 - f0) (t1 - t0) HOST doubles,
 * brought by the call's one synchronisation.  weights: the block's shape, real of that precision, or NULL (every weight
 * 1); inverse variances, 0 flags a sample with fv_weight_rows' rules.  weights_on_device as in fv_sim_run_residual; host
 * weights are staged on the device, and their bytes are given back under the FFTVIS_HIP_ADJ_KEEP_BYTES rule of
 * fv_sim_run_adjoint.  parts_dev[0] is then what every fv_sim_run_*_adjoint of this handle takes as its input: H p of the
 * Gauss-Newton Hessian H = 2 J^T W J of fv_sim_run_residual's chi2.  The rows' sums are bitwise reproducible for given
 * parts.  A null handle, nparts outside 1 .. 4, a null part or q_ft, a flag other than 0 or 1 and an empty range fail with
 * FV_ERR_ARG before anything runs; a weight that is negative or not finite fails the call with FV_ERR_ARG after it ran
 * (counted by the kernel itself): parts_dev[0] and q_ft are then invalid and the handle stays usable.                     */
int fv_sim_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, const void *weights,
                        int weights_on_device, double *q_ft);
/* fv_sim_weight_block with per-antenna gains and a gain direction: the Gauss-Newton product of
 * fv_sim_run_residual_gains' chi2.  The call is fv_sim_weight_block's -- kernels on the main stream, one synchronisation
 * -- with the two kernels of fv_gain_weight_rows, whose formulas hold element by element: parts_dev are nparts = 0 .. 4
 * DEVICE tangent blocks, vis_dev the DEVICE block fv_sim_run wrote at the real parameters (needed with d_gains, with
 * hgains and for nparts = 0; else it may be NULL), and  stored G = conj(m) G',  G' = 2 (w U'),  U' = m U + dm V,  is left
 * in parts_dev[0] (in vis_dev for nparts = 0): what every fv_sim_run_*_adjoint of this handle takes as its input.  q_ft
 * as for fv_sim_weight_block, the rows of sum w |U'|^2.  gains, d_gains: (f1 - f0, t1 - t0, nfeed, nant) complex of the
 * handle's precision, d_gains or NULL; hgains: the same shape in complex128, the gain block of H p, or NULL.  Host gains,
 * direction and hgains are staged and given back with host weights under the FFTVIS_HIP_ADJ_KEEP_BYTES rule.  Needs
 * fv_sim_set_gain_pairs.  A null handle, nparts outside 0 .. 4, nparts = 0 without d_gains, a null part, gains or q_ft,
 * d_gains or hgains without vis_dev, a flag other than 0 or 1, an empty range and missing pairs fail with FV_ERR_ARG
 * before anything runs; bad weights as for fv_sim_weight_block.                                                          */
int fv_sim_gain_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                             const void *weights, int weights_on_device, const void *gains, int gains_on_device,
                             const void *d_gains, int d_gains_on_device, double *q_ft, void *hgains, int hgains_on_device);
/* fv_sim_gain_weight_block with one 2 x 2 complex (Jones) matrix per antenna and a direction of such matrices: the
 * Gauss-Newton product of fv_sim_run_residual_jones' chi2, on a polarized handle.  The call is fv_sim_gain_weight_block's,
 * argument for argument, with the two kernels of fv_jones_weight_rows, whose formulas hold baseline by baseline: the stored
 * G of G' = 2 (w U') is left in parts_dev[0] (in vis_dev for nparts = 0), q_ft are the rows of sum w |U'|^2.  jones,
 * d_jones: (f1 - f0, t1 - t0, 2, 2, nant) complex of the handle's precision, d_jones or NULL; hjones: the same shape in
 * complex128, the matrices' block of H p, or NULL.  The device holds one more fp64 value per value of the block (the rows'
 * terms).  Host matrices, direction and hjones are staged and given back with host weights under the
 * FFTVIS_HIP_ADJ_KEEP_BYTES rule.  Needs fv_sim_set_gain_pairs.  A null handle, nparts outside 0 .. 4, nparts = 0 without
 * d_jones, a null part, jones or q_ft, d_jones or hjones without vis_dev, a flag other than 0 or 1, an empty range, missing
 * pairs and an unpolarized handle fail with FV_ERR_ARG before anything runs; bad weights as for fv_sim_weight_block.      */
int fv_sim_jones_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                              const void *weights, int weights_on_device, const void *jones, int jones_on_device,
                              const void *d_jones, int d_jones_on_device, double *q_ft, void *hjones, int hjones_on_device);
/* Which transform fv_sim_run_adjoint uses on a lattice handle (fv_sim_set_array_type1; the forward there is the type-1
 * transform of src/fftvis/cpu/nufft.py:120-175, chosen at cpu_simulate.py:634-637).  path 0 (default): the type-3
 * transform with the roles swapped, as on every other array.  path 1: the transpose of the type-1 slice itself, a type-2
 * transform -- the runs' strengths go to their integer modes (deconvolved, as :259-269 picks them), the forward's n2 x n2
 * planes are transformed the other way round (n_modes + 1 inputs, every output) and gathered periodically at the
 * (source, channel) entries the forward spreads from; frequency batches as in fv_sim_run (FFTVIS_HIP_GRID_BYTES).  Both
 * compute the same map to the handle's tolerance.  The setting stays with the handle.  Any other value fails with
 * FV_ERR_ARG; path 1 on a handle that is not a lattice handle fails the next fv_sim_run_adjoint with FV_ERR_ARG.          */
int fv_sim_set_adjoint_path(fv_sim *h, int path);
/* The transform the last successful fv_sim_run_adjoint of this handle took: 0 none yet, 2 the type-2 transform, 3 the
 * type-3 transform.  A null handle returns FV_ERR_ARG (1), which is none of these.                                        */
int fv_sim_last_adjoint_path(fv_sim *h);
int fv_sim_sync(fv_sim *h);

/* Introspection for bench/roofline: fills up to n doubles:
 * [0] spread launches, counted per (time, frequency group, beam pair) -- a gang launch that serves two
 * time steps counts twice, and a launch's transforms may run as several kernel launches --, [1] fine-grid cells written by spread (all trans, summed),
 * [2] source x trans visits, [3] cells moved through HBM by the pruned FFT passes,
 * [4] gathered footprints (targets x transforms, x 2 for packed transforms: read at s and -s), [5] above-horizon sources summed over times, [6] last n2x,
 * [7] last n2y, [8] last (na_x * 65536 + na_y), [9] kernel width w, [10] upsampling factor the
 * last run used, [11] largest above-horizon source count of any time step since the reset, [12] real flops of the FFT
 * passes priced as plain transforms (5 n2 log2 n2 per line transformed), [13] last n2 of the third dimension (1 for
 * 2-D runs), [14] last na of the third dimension, [15] height terms of the last run (K > 0: a non-coplanar array ran
 * as K 2-D transforms per slice, the expansion of exp(i z s_z) about the middle of the sources' height range; 0: no
 * expansion -- coplanar, or the 3-D transform), [16] lanes of the last type-3 run (2: consecutive time steps alternate
 * between two sets of scratch and grid buffers), [17] how they ran: 0 freely on two streams of equal priority (large
 * grids: the kernels of two time steps share the GPU, and kernel durations are those of kernels sharing it), 1
 * pipelined (big kernels in order on one stream, the next step's preparation beside them), 2 pipelined gangs,
 * [18] first LIGHT height term of the last run (terms k >= this ran on a second plan at a looser tolerance and
 * upsampling factor 1.25: they enter with weights 2 |J_k|; 0: none), [19] first term of a second, looser light class
 * (0: one class).                                                                                                   */
int fv_sim_stats(fv_sim *h, double *vals, int n);
int fv_sim_reset_stats(fv_sim *h);
/* HIP-event timing on the handle's stream (ms, summed since reset): [0] spread, [1] fft,
 * [2] interp, [3] strengths (beam + coherency), [4] rotate/sort, [5] number of spread launches
 * behind [0].  level 0: off; 1: spread only, events attached to the dispatches themselves (no extra
 * queue packets) for the spread launches of one time step in 16 of a run (the 9th: steady state) -- sampled because even
 * attached events idle the queue for a few us around a launch; cheap enough for a timed region; 2: every launch of every
 * family, bracketed by event records (adds ~10 us bubbles each; runs on a single stream); 3: as 1 but on
 * every spread launch (large grids, where a launch is hundreds of us and the bubble does not matter). */
int fv_sim_enable_timing(fv_sim *h, int level);
int fv_sim_timing(fv_sim *h, double *ms, int n);

/* ---- catalog exchange over RCCL (optional; SURVEY 8 b "fv_comm_init / fv_bcast_catalog", 8 e) ---------------------
 * For hosts that do not bring torch.distributed: the path's only exchange step is one broadcast of the catalog from the
 * rank that read it (the reference ships it to its Ray workers as a whole, cpu_simulate.py:711-847 via core/utils.py:
 * 122-187) -- positions to everyone, flux either whole (fv_bcast_catalog) or only the frequency columns of each rank's
 * block (fv_scatter_flux_columns: one packed ncclSend per rank in one group; C3 on 8 ranks: 32 instead of 250 MB per
 * rank).  Buffers are DEVICE pointers on the communicator's GPU; what arrives goes to fv_sim_set_sources(...,
 * on_device = 1).  Visibilities are never exchanged: every rank copies its own block out (fv_sim_run / fv_sim_run_into).
 * librccl.so.1 is opened on first use: without it these five entries fail with FV_ERR_INTERNAL and nothing else changes.
 *   fv_comm_unique_id : rank 0 fills FV_COMM_ID_BYTES bytes (ncclGetUniqueId); the host carries them to the other ranks
 *   fv_comm_init      : collective over the nranks processes (ncclCommInitRank), one process per GPU
 *   fv_bcast_catalog  : eq (3, nsrc) and flux as fv_sim_set_sources lays them out, as bytes; in place on every rank
 *   fv_scatter_flux_columns : flux_root_dev (nsrc, nfreq) entries of elem_bytes (8: float64, 4: float32, 64 / 32:
 *       2 x 2 complex) on the root; ranges = nranks pairs [f0, f1); out_dev (nsrc, f1 - f0) of THIS rank
 * Both transfers return after the data has arrived (the communicator's stream is synchronised).
 * Verified on hardware with one rank only (a one-GPU box cannot host two RCCL ranks); the Python host's
 * torch.distributed path (parallel.broadcast_catalog_device) is the one the multi-process tests cover.            */
#define FV_COMM_ID_BYTES 128
typedef struct fv_comm fv_comm;
int fv_comm_unique_id(void *id_bytes);
int fv_comm_init(fv_comm **c, int device, int rank, int nranks, const void *id_bytes);
int fv_comm_destroy(fv_comm *c);
int fv_bcast_catalog(fv_comm *c, int root, void *eq_dev, int64_t eq_bytes, void *flux_dev, int64_t flux_bytes);
int fv_scatter_flux_columns(fv_comm *c, int root, int64_t nsrc, int nfreq, int elem_bytes, const void *flux_root_dev,
                            const int *ranges, void *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* FFTVIS_HIP_H */
