// fv_capi.hip -- extern "C" entry points of libfftvis_hip.so (see include/fftvis_hip.h).
// Single translation unit: hipcc --offload-arch=gfx950 -O3 -shared -fPIC ...

#include "../../include/fftvis_hip.h"
#include "fv_sim.h"

#include <algorithm>
#include <atomic>
#include <mutex>

namespace fv {

static thread_local std::string g_last_error;

template <typename F>
static int guarded(F &&f) {
    try {
        f();
        return FV_OK;
    } catch (const Error &e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return FV_ERR_INTERNAL;
    } catch (...) {
        g_last_error = "unknown error";
        return FV_ERR_INTERNAL;
    }
}

// What the entry points' checks share.  f(T{}), T the real type of `precision`: a body is written once for both
template <typename F>
static void with_precision(int precision, F &&f) {
    FV_REQUIRE(precision == 1 || precision == 2, "precision must be 1 or 2");
    if (precision == 1)
        f(float{});
    else
        f(double{});
}
template <typename F>
static int guarded(int precision, F &&f) {
    return guarded([&] { with_precision(precision, f); });
}
static void require_on_device_flags(std::initializer_list<int> flags) {
    int bits = 0;
    for (int f : flags) bits |= f;
    FV_REQUIRE((bits & ~1) == 0, "on_device flags must be 0 or 1");
}
// every baseline's antenna pair lies in [0, nant); `entry` names the caller in the message
static void require_pairs(const char *entry, int64_t nbls, int nant, const int *ant1, const int *ant2) {
    for (int64_t k = 0; k < nbls; ++k)
        FV_REQUIRE(ant1[k] >= 0 && ant1[k] < nant && ant2[k] >= 0 && ant2[k] < nant,
                   std::string(entry) + ": antenna index outside [0, nant)");
}

struct StreamGuard {
    hipStream_t s = nullptr;
    StreamGuard() { FV_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~StreamGuard() {
        if (s) (void)hipStreamDestroy(s);
    }
};

static void minmax(const double *v, int64_t n, double &c, double &h) {
    double lo = 1e300, hi = -1e300;
    for (int64_t i = 0; i < n; ++i) {
        lo = std::min(lo, v[i]);
        hi = std::max(hi, v[i]);
    }
    if (n == 0) lo = hi = 0;
    c = 0.5 * (lo + hi);
    h = 0.5 * (hi - lo);
    // guard the box against the T-rounding of the uploaded coordinates
    h = h * (1.0 + 1e-6) + 1e-300;
}

// Stream, device buffers and plan of the stand-alone transform, kept per host thread between calls
// with the same (device, dim, eps, upsampling factor): setting them up costs ~5 ms, more than a small
// transform.  Held through plain pointers that only fv_release_workspaces() deletes (static
// destructors must not call into a HIP runtime that may be gone); dropped after a call that leaves the
// process above FFTVIS_HIP_HANDLE_CACHE_BYTES (default 2 GiB) of device memory.
template <typename T>
struct NufftWorkspace {
    int device = -1, dim = 0;
    double eps = 0, sigma = 0;
    uint64_t id = 0;  // unique over the life of the process: a thread's slot is (pointer, id), so a workspace that
                      // another thread freed and a NEW one that happens to sit at the same address never compare equal
    hipStream_t st = nullptr;
    DevBuf dx[3], ds[3], dc, dout, dscale;
    std::unique_ptr<Nufft3<T>> plan;
    ~NufftWorkspace() {
        plan.reset();
        if (st) (void)hipStreamDestroy(st);
    }
};
template <typename T>
static NufftWorkspace<T> *&workspace_slot() {
    static thread_local NufftWorkspace<T> *ws = nullptr;
    return ws;
}
template <typename T>
static uint64_t &workspace_slot_id() {
    static thread_local uint64_t id = 0;
    return id;
}
static uint64_t next_workspace_id() {
    static std::atomic<uint64_t> n{0};
    return ++n;
}
// Every live workspace, whichever thread made it, so that fv_release_workspaces() can free those of
// threads that have exited (their thread_local pointer died with them, the device memory did not).
// A thread's slot holds an index into this registry rather than ownership.
template <typename T>
struct WorkspaceRegistry {
    std::mutex mu;
    std::vector<NufftWorkspace<T> *> all;
    static WorkspaceRegistry &get() {
        static WorkspaceRegistry *r = new WorkspaceRegistry();  // never destroyed: see the note above
        return *r;
    }
    void add(NufftWorkspace<T> *w) {
        std::lock_guard<std::mutex> g(mu);
        all.push_back(w);
    }
    bool remove(NufftWorkspace<T> *w) {  // true if it was still registered (i.e. nobody freed it yet)
        std::lock_guard<std::mutex> g(mu);
        auto it = std::find(all.begin(), all.end(), w);
        if (it == all.end()) return false;
        all.erase(it);
        return true;
    }
    bool contains(NufftWorkspace<T> *w, uint64_t id) {  // registered AND the same object the slot was made for
        std::lock_guard<std::mutex> g(mu);
        auto it = std::find(all.begin(), all.end(), w);
        return it != all.end() && (*it)->id == id;
    }
    bool remove(NufftWorkspace<T> *w, uint64_t id) {
        std::lock_guard<std::mutex> g(mu);
        auto it = std::find(all.begin(), all.end(), w);
        if (it == all.end() || (*it)->id != id) return false;
        all.erase(it);
        return true;
    }
    void drain() {
        std::vector<NufftWorkspace<T> *> take;
        {
            std::lock_guard<std::mutex> g(mu);
            take.swap(all);
        }
        for (NufftWorkspace<T> *w : take) {
            (void)hipSetDevice(w->device);
            delete w;
        }
    }
};
static size_t workspace_limit() {
    const char *e = std::getenv("FFTVIS_HIP_HANDLE_CACHE_BYTES");
    return e ? (size_t)std::atof(e) : ((size_t)2 << 30);
}
template <typename T>
static void drop_workspace() {
    NufftWorkspace<T> *&ws = workspace_slot<T>();
    if (ws) {
        if (WorkspaceRegistry<T>::get().remove(ws, workspace_slot_id<T>())) {  // else another thread's fv_release_workspaces() freed it
            (void)hipSetDevice(ws->device);
            delete ws;
        }
        ws = nullptr;
    }
}

template <typename T>
static void nufft3_host(int device, int dim, int64_t M, const void *const xin[3], const void *cin,
                        int ntrans, int64_t N, const void *const sin_[3], double eps,
                        double upsampfac, void *out, bool direct) {
    FV_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
    FV_REQUIRE(M >= 0 && N >= 0 && ntrans >= 1, "negative sizes");
    for (int d = 0; d < dim; ++d)
        FV_REQUIRE((xin[d] || M == 0) && (sin_[d] || N == 0), "missing coordinate array");
    FV_REQUIRE(cin || M == 0, "missing strengths");
    FV_REQUIRE(out || N == 0, "missing output");
    FV_HIP(hipSetDevice(device));
    if (N == 0) return;
    if (M == 0) {
        std::memset(out, 0, sizeof(cplx<T>) * (size_t)ntrans * N);
        return;
    }
    NufftWorkspace<T> *&slot = workspace_slot<T>();
    if (slot && !WorkspaceRegistry<T>::get().contains(slot, workspace_slot_id<T>())) slot = nullptr;  // freed by another thread's release
    if (slot && (slot->device != device || slot->dim != dim || slot->eps != eps || slot->sigma != upsampfac))
        drop_workspace<T>();
    if (!slot) {
        slot = new NufftWorkspace<T>();
        slot->device = device;
        slot->dim = dim;
        slot->eps = eps;
        slot->sigma = upsampfac;
        slot->id = workspace_slot_id<T>() = next_workspace_id();
        FV_HIP(hipStreamCreateWithFlags(&slot->st, hipStreamNonBlocking));
        WorkspaceRegistry<T>::get().add(slot);
    }
    struct DropOnError {  // an exception may leave the plan half configured
        bool armed = true;
        ~DropOnError() {
            if (armed) drop_workspace<T>();
        }
    } guard;
    NufftWorkspace<T> &W = *slot;
    hipStream_t st = W.st;
    DevBuf(&dx)[3] = W.dx, (&ds)[3] = W.ds, &dc = W.dc, &dout = W.dout, &dscale = W.dscale;
    double xc[3] = {0, 0, 0}, X[3] = {0, 0, 0}, sc[3] = {0, 0, 0}, S[3] = {0, 0, 0};
    std::vector<double> tmp;
    for (int d = 0; d < dim; ++d) {
        tmp.resize(std::max(M, N));
        const T *xv = (const T *)xin[d];
        for (int64_t i = 0; i < M; ++i) tmp[i] = xv[i];
        minmax(tmp.data(), M, xc[d], X[d]);
        const T *sv = (const T *)sin_[d];
        for (int64_t i = 0; i < N; ++i) tmp[i] = sv[i];
        minmax(tmp.data(), N, sc[d], S[d]);
        dx[d].reserve(sizeof(T) * M);
        ds[d].reserve(sizeof(T) * N);
        FV_HIP(hipMemcpyAsync(dx[d].p, xin[d], sizeof(T) * M, hipMemcpyHostToDevice, st));
        FV_HIP(hipMemcpyAsync(ds[d].p, sin_[d], sizeof(T) * N, hipMemcpyHostToDevice, st));
    }
    dc.reserve(sizeof(cplx<T>) * (size_t)ntrans * M);
    dout.reserve(sizeof(cplx<T>) * (size_t)ntrans * N);
    FV_HIP(hipMemcpyAsync(dc.p, cin, sizeof(cplx<T>) * (size_t)ntrans * M, hipMemcpyHostToDevice, st));

    if (direct) {
        hipLaunchKernelGGL(k_nudft_direct<T>, dim3((unsigned)N, (unsigned)ntrans), dim3(256), 0, st,
                           dim, M, dx[0].as<T>(), dx[1].as<T>(), dx[2].as<T>(), dc.as<cplx<T>>(),
                           ntrans, N, ds[0].as<T>(), ds[1].as<T>(), ds[2].as<T>(),
                           dout.as<cplx<T>>());
    } else {
        const double one = 1.0;
        dscale.reserve(sizeof(double));
        FV_HIP(hipMemcpyAsync(dscale.p, &one, sizeof(double), hipMemcpyHostToDevice, st));
        if (!W.plan) W.plan.reset(new Nufft3<T>(dim, eps, upsampfac, st));
        Nufft3<T> &plan = *W.plan;
        plan.set_geometry(xc, X, sc, S, 1.0);
        plan.set_sources(M, dx[0].as<T>(), dx[1].as<T>(), dx[2].as<T>());
        plan.load_strengths(dc.as<cplx<T>>(), ntrans, ntrans, dscale.as<double>());
        plan.spread(ntrans);
        plan.fft(ntrans);
        int64_t pol_off[16];
        for (int r = 0; r < 16; ++r) pol_off[r] = (int64_t)r * N;
        plan.interp(N, ds[0].as<T>(), ds[1].as<T>(), ds[2].as<T>(), nullptr, nullptr,
                    dscale.as<double>(), 1, ntrans, dout.as<cplx<T>>(), 0, 1, pol_off, false);
        FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(cplx<T>) * (size_t)ntrans * N,
                              hipMemcpyDeviceToHost, st));
        FV_HIP(hipStreamSynchronize(st));
        FV_HIP(hipGetLastError());
        // finufft rejects points it cannot place; here they were clamped to an edge cell and counted
        const int noob = plan.out_of_box_count();
        FV_REQUIRE(noob == 0, std::to_string(noob) + " source coordinates are NaN or outside the box of the "
                                                       "finite ones: the transform is invalid");
        guard.armed = fv::dev_bytes_held().load() > workspace_limit();
        return;
    }
    FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(cplx<T>) * (size_t)ntrans * N, hipMemcpyDeviceToHost, st));
    FV_HIP(hipStreamSynchronize(st));
    FV_HIP(hipGetLastError());
    guard.armed = fv::dev_bytes_held().load() > workspace_limit();
}

template <typename T>
static void beam_eval_host(int device, int polarized, int kind, double diameter, int nft, int nza,
                           int naz, double za_max, const void *table, int order, int fidx, double freq,
                           int64_t n, const void *az, const void *za, void *out) {
    FV_REQUIRE(kind == 0 || kind == 1, "beam kind must be 0 (Airy) or 1 (table)");
    FV_REQUIRE(order >= 0 && order <= 5, "beam interpolation order must be 0 .. 5");
    FV_REQUIRE(n >= 0 && (n == 0 || (az && za && out)), "bad beam_eval arrays");
    FV_HIP(hipSetDevice(device));
    if (n == 0) return;
    StreamGuard sg;
    DevBuf daz, dza, dout, dtab, dtab_in;
    BeamDesc b{};
    b.kind = kind;
    b.diameter = diameter;
    for (int i = 0; i < 8; ++i) b.js[i] = i % 2 ? 0.0 : 1.0;
    b.ps = 1.0;
    if (kind == 0 && table) {  // Airy with factors: 8 doubles (Jones slots, re / im) + the power factor
        const double *f = static_cast<const double *>(table);
        for (int i = 0; i < 8; ++i) b.js[i] = f[i];
        b.ps = f[8];
    }
    if (kind == 1) {
        FV_REQUIRE(table && nza >= 2 && naz >= 1 && nft >= 1 && za_max > 0, "bad beam table");
        FV_REQUIRE(nft == 1 || (fidx >= 0 && fidx < nft), "freq_index outside the beam table");
        const size_t bytes = (polarized ? 64 : 8) * (size_t)nft * nza * naz;
        dtab.reserve(bytes);
        if (!polarized) {
            FV_HIP(hipMemcpyAsync(dtab.p, table, bytes, hipMemcpyHostToDevice, sg.s));
        } else {  // Jones tables are read in the interleaved device layout (eval_jones)
            dtab_in.reserve(bytes);
            FV_HIP(hipMemcpyAsync(dtab_in.p, table, bytes, hipMemcpyHostToDevice, sg.s));
            const int64_t nodes = (int64_t)nza * naz;
            hipLaunchKernelGGL(k_jones_interleave, dim3((unsigned)cdiv(nodes * nft, 256)), dim3(256), 0, sg.s,
                               dtab_in.as<cplx<double>>(), dtab.as<cplx<double>>(), nodes, (int64_t)nft);
        }
        bspline_prefilter(dtab.as<double>(), nft, nza, naz, polarized ? 8 : 1, order, sg.s);
        b.order = order;
        b.table = dtab.p;
        b.nfreq_tab = nft;
        b.nza = nza;
        b.naz = naz;
        b.za_max = za_max;
    } else {
        FV_REQUIRE(diameter > 0, "diameter must be positive");
    }
    const size_t nout = (polarized ? 4 : 1) * (size_t)n;
    daz.reserve(sizeof(T) * n);
    dza.reserve(sizeof(T) * n);
    dout.reserve(sizeof(cplx<T>) * nout);
    FV_HIP(hipMemcpyAsync(daz.p, az, sizeof(T) * n, hipMemcpyHostToDevice, sg.s));
    FV_HIP(hipMemcpyAsync(dza.p, za, sizeof(T) * n, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL((order == 3 ? k_beam_eval<T, 3> : order == 1 ? k_beam_eval<T, 1> : k_beam_eval<T, 0>), dim3(cdiv(n, 256)), dim3(256), 0, sg.s, b, polarized, fidx,
                       freq, n, daz.as<T>(), dza.as<T>(), dout.as<cplx<T>>());
    FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(cplx<T>) * nout, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

template <typename T>
static void coherency_host(int device, int variant, int64_t n, const void *bi, const void *bj,
                           const void *flux, void *out) {
    FV_REQUIRE(variant >= 0 && variant <= 4, "coherency variant must be 0..4");
    FV_REQUIRE(n >= 0 && (n == 0 || (bi && bj && flux && out)), "bad coherency arrays");
    FV_HIP(hipSetDevice(device));
    if (n == 0) return;
    StreamGuard sg;
    const size_t nb = (variant == 4 ? 1 : 4) * (size_t)n;
    const bool cflux = variant == 1 || variant == 3;
    const size_t fbytes = cflux ? sizeof(cplx<T>) * 4 * n : sizeof(T) * n;
    DevBuf dbi, dbj, dfl, dout;
    dbi.reserve(sizeof(cplx<T>) * nb);
    dbj.reserve(sizeof(cplx<T>) * nb);
    dfl.reserve(fbytes);
    dout.reserve(sizeof(cplx<T>) * nb);
    FV_HIP(hipMemcpyAsync(dbi.p, bi, sizeof(cplx<T>) * nb, hipMemcpyHostToDevice, sg.s));
    FV_HIP(hipMemcpyAsync(dbj.p, bj, sizeof(cplx<T>) * nb, hipMemcpyHostToDevice, sg.s));
    FV_HIP(hipMemcpyAsync(dfl.p, flux, fbytes, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(k_apparent_coherency<T>, dim3(cdiv(n, 256)), dim3(256), 0, sg.s, variant, n,
                       dbi.as<cplx<T>>(), dbj.as<cplx<T>>(), dfl.p, dout.as<cplx<T>>());
    FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(cplx<T>) * nb, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

// The row passes on host arrays (fv_residual_chi2, fv_gain_residual_chi2, fv_jones_residual_chi2, fv_weight_rows,
// fv_gain_weight_rows, fv_jones_weight_rows): every array is copied into a buffer of its own on the call's stream (null
// stays null), the launcher queues the kernels, what was computed in place is copied back and collect_rows ends the call.
template <typename X>
static X *to_device(hipStream_t s, DevBuf &buf, const void *host, size_t n) {
    if (!host) return nullptr;
    buf.reserve(sizeof(X) * n);
    FV_HIP(hipMemcpyAsync(buf.p, host, sizeof(X) * n, hipMemcpyHostToDevice, s));
    return buf.as<X>();
}
// a call's calibration as the caller gave it: the pairs, the rows' gains or matrices x, their direction dx (or null) and
// where the gradient goes (complex128, the shape of x; or null)
struct HostCal {
    Cal kind = Cal::None;
    int tpol = 1, nant = 0;
    int64_t nbls = 0;
    const int *ant1 = nullptr, *ant2 = nullptr;
    const void *x = nullptr, *dx = nullptr;
    void *grad = nullptr;
};
// ... and on the device, for a block of n values with nx entries of x: the pairs of this call, x and dx copied, the
// gradient's block and (Jones) the rows' terms reserved
template <typename T>
struct DeviceCal {
    GainPairs gp;
    DevBuf dx, ddx, dgrad, dterms;
    RowCal<T> cal;
    DeviceCal(hipStream_t s, const HostCal &c, size_t n, size_t nx) {
        if (c.kind == Cal::None) return;
        gp.set(s, c.nant, c.nbls, c.ant1, c.ant2);
        if (c.grad) dgrad.reserve(sizeof(cplx<double>) * nx);
        if (c.kind == Cal::Jones) dterms.reserve(sizeof(double) * n);
        cal = {c.kind, &gp, to_device<cplx<T>>(s, dx, c.x, nx), to_device<cplx<T>>(s, ddx, c.dx, nx), dgrad.as<cplx<double>>(),
               dterms.as<double>()};
    }
};
// what both passes do with an empty block (true: done): no rows, or rows of no values, whose sums and gradient are zero
static bool empty_rows(int64_t nrows, int64_t row_len, double *rows, void *grad, size_t nx) {
    if (nrows > 0 && row_len == 0) {
        for (int64_t i = 0; i < nrows; ++i) rows[i] = 0.0;
        if (grad) std::memset(grad, 0, sizeof(cplx<double>) * nx);
    }
    return nrows == 0 || row_len == 0;
}
// ... and at their end: the gradient's block and the rows' sums come back, and bad input is reported
template <typename T>
static void finish_rows_host(hipStream_t s, const DeviceCal<T> &dc, void *grad, size_t nx, const RowScratch &rs, int64_t nrows,
                             double *rows) {
    if (grad) FV_HIP(hipMemcpyAsync(grad, dc.dgrad.p, sizeof(cplx<double>) * nx, hipMemcpyDeviceToHost, s));
    int hbad[2];
    collect_rows(s, rs, nrows, rows, hbad);
    throw_if_bad_residual_input(hbad);
}

template <typename T>
static void residual_rows_host(int device, int64_t nrows, int64_t row_len, void *vis, const void *data, const void *weights,
                               double *chi2_rows, const HostCal &c = {}) {
    const size_t n = (size_t)nrows * (size_t)row_len, nx = (size_t)nrows * (size_t)cal_entries(c.kind, c.tpol, c.nant);
    if (empty_rows(nrows, row_len, chi2_rows, c.grad, nx)) return;
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    DeviceCal<T> dc(sg.s, c, n, nx);
    DevBuf dv, dd, dw, ds;
    const RowScratch rs = row_scratch<T>(ds, nrows, row_len);
    launch_residual<T>(sg.s, to_device<cplx<T>>(sg.s, dv, vis, n), to_device<cplx<T>>(sg.s, dd, data, n),
                       to_device<T>(sg.s, dw, weights, n), nrows, row_len, rs, dc.cal);
    FV_HIP(hipMemcpyAsync(vis, dv.p, sizeof(cplx<T>) * n, hipMemcpyDeviceToHost, sg.s));
    finish_rows_host(sg.s, dc, c.grad, nx, rs, nrows, chi2_rows);
}

template <typename T>
static void weight_rows_host(int device, int64_t nrows, int64_t row_len, int nparts, const void *const *parts, void *vis,
                             const void *weights, double *q_rows, const HostCal &c = {}) {
    const size_t n = (size_t)nrows * (size_t)row_len, nx = (size_t)nrows * (size_t)cal_entries(c.kind, c.tpol, c.nant);
    if (empty_rows(nrows, row_len, q_rows, c.grad, nx)) return;
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    DeviceCal<T> dc(sg.s, c, n, nx);
    DevBuf dp[4], dv, dw, ds;
    cplx<T> *dparts[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < nparts; ++j) dparts[j] = to_device<cplx<T>>(sg.s, dp[j], parts[j], n);
    const RowScratch rs = row_scratch<T>(ds, nrows, row_len);
    launch_weight_rows<T>(sg.s, nparts, dparts, to_device<cplx<T>>(sg.s, dv, vis, n), to_device<T>(sg.s, dw, weights, n), nrows,
                          row_len, rs, dc.cal);
    if (nparts)  // G replaces P_0, or V for the direction of the gains or matrices alone
        FV_HIP(hipMemcpyAsync(const_cast<void *>(parts[0]), dp[0].p, sizeof(cplx<T>) * n, hipMemcpyDeviceToHost, sg.s));
    else
        FV_HIP(hipMemcpyAsync(vis, dv.p, sizeof(cplx<T>) * n, hipMemcpyDeviceToHost, sg.s));
    finish_rows_host(sg.s, dc, c.grad, nx, rs, nrows, q_rows);
}

template <typename T>
static void gain_normal_rows_host(int device, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1, const int *ant2,
                                  const void *gains, const void *vis, const void *data, const void *weights, void *num, double *den) {
    const int nfeed = tpol == 4 ? 2 : 1;
    const size_t ng = (size_t)nrows * nfeed * (size_t)nant;
    if (nrows == 0) return;
    if (nbls == 0) {
        std::memset(num, 0, sizeof(cplx<double>) * ng);
        std::memset(den, 0, sizeof(double) * ng);
        return;
    }
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nrows * (size_t)tpol * (size_t)nbls;
    GainPairs gp;
    gp.set(sg.s, nant, nbls, ant1, ant2);
    DevBuf dv, dd, dw, dgn, dnum, dden;
    dv.reserve(sizeof(cplx<T>) * n);
    dd.reserve(sizeof(cplx<T>) * n);
    if (weights) dw.reserve(sizeof(T) * n);
    dgn.reserve(sizeof(cplx<double>) * ng);
    dnum.reserve(sizeof(cplx<double>) * ng);
    dden.reserve(sizeof(double) * ng);
    FV_HIP(hipMemcpyAsync(dv.p, vis, sizeof(cplx<T>) * n, hipMemcpyHostToDevice, sg.s));
    FV_HIP(hipMemcpyAsync(dd.p, data, sizeof(cplx<T>) * n, hipMemcpyHostToDevice, sg.s));
    if (weights) FV_HIP(hipMemcpyAsync(dw.p, weights, sizeof(T) * n, hipMemcpyHostToDevice, sg.s));
    FV_HIP(hipMemcpyAsync(dgn.p, gains, sizeof(cplx<double>) * ng, hipMemcpyHostToDevice, sg.s));
    launch_gain_normal<T>(sg.s, dv.as<cplx<T>>(), dd.as<cplx<T>>(), weights ? dw.as<T>() : nullptr, dgn.as<cplx<double>>(), gp, nrows,
                          1, tpol, dnum.as<cplx<double>>(), dden.as<double>(), nullptr);
    FV_HIP(hipMemcpyAsync(num, dnum.p, sizeof(cplx<double>) * ng, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(den, dden.p, sizeof(double) * ng, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

// The alternating solve that fv_gain_solve and fv_jones_solve run (DESIGN.md "Gain solve", "Jones solve"): device blocks
// are used where they lie, host blocks are staged once; the iterate lives in two device buffers and only the units' change
// comes back per iteration.  What differs comes from the caller: the values of a row (row_len), the complex128 entries
// of a unit's iterate (nx) and the ints of its `solved` (ns), the bytes a row's normal sums take in the two scratch
// buffers, the partials per row of the chi2 pass (npart doubles, in the first scratch buffer), and the three launches.
struct SolveBlocks {  // what the launches are given: all device pointers, weights may be null
    hipStream_t on;
    const GainPairs &gp;
    const void *vis, *data, *weights;
    int64_t nrows, rows_per_unit;
    void *sums0, *sums1;
};
template <typename T, typename Normal, typename Update, typename Chi2>
static void alternating_solve(int device, int nfreqs, int ntimes, int64_t nbls, int nant, const int *ant1, const int *ant2, int per_time,
                              int64_t row_len, int nx, int ns, size_t row_bytes0, size_t row_bytes1, int npart, const void *vis,
                              int vis_on_device, const void *data, int data_on_device, const void *weights, int weights_on_device,
                              void *x, int max_iter, double tol, int *niter_out, double *change_out, double *chi2_ft_out,
                              int *solved_out, Normal normal, Update update, Chi2 chi2) {
    const int64_t nrows = (int64_t)nfreqs * ntimes, rows_per_unit = per_time ? 1 : ntimes;
    const int64_t nunits = per_time ? nrows : nfreqs;
    *niter_out = 0;
    if (nrows == 0) return;  // (no unit: the iterate, change and solved are empty)
    std::fill(change_out, change_out + nunits, 0.0);
    std::fill(chi2_ft_out, chi2_ft_out + nrows, 0.0);
    std::fill(solved_out, solved_out + nunits * ns, 0);
    if (nbls == 0) return;  // (the start, chi2 0, nothing solved)
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nrows * (size_t)row_len, nxu = (size_t)nunits * nx, nsu = (size_t)nunits * ns;
    GainPairs gp;
    gp.set(sg.s, nant, nbls, ant1, ant2);
    DevBuf sv, sd, sw, dx[2], sums0, sums1, dchange, dsolved, dchi2, dbad;
    const auto staged = [&](DevBuf &buf, const void *x, int on_device, size_t bytes) -> const void * {
        if (!x || on_device) return x;
        buf.reserve(bytes);
        FV_HIP(hipMemcpyAsync(buf.p, x, bytes, hipMemcpyHostToDevice, sg.s));
        return buf.p;
    };
    const cplx<T> *dv = static_cast<const cplx<T> *>(staged(sv, vis, vis_on_device, sizeof(cplx<T>) * n));
    const cplx<T> *dd = static_cast<const cplx<T> *>(staged(sd, data, data_on_device, sizeof(cplx<T>) * n));
    const T *dw = static_cast<const T *>(staged(sw, weights, weights_on_device, sizeof(T) * n));
    for (auto &b : dx) b.reserve(sizeof(cplx<double>) * nxu);
    sums0.reserve(row_bytes0 * (size_t)nrows);
    sums1.reserve(row_bytes1 * (size_t)nrows);
    dchange.reserve(sizeof(double) * (size_t)nunits);
    dsolved.reserve(sizeof(int) * nsu);
    dchi2.reserve(sizeof(double) * (size_t)nrows);
    dbad.reserve(16);
    FV_HIP(hipMemcpyAsync(dx[0].p, x, sizeof(cplx<double>) * nxu, hipMemcpyHostToDevice, sg.s));
    int *bad = dbad.as<int>();
    int hbad[3] = {0, 0, 0};
    FV_HIP(hipMemsetAsync(bad, 0, sizeof(hbad), sg.s));
    hipLaunchKernelGGL(k_gain_solve_check<T>, dim3((unsigned)std::min<int64_t>(cdiv((int64_t)n, 256), 4096)), dim3(256), 0, sg.s, dv, dd,
                       dw, gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), (int64_t)n, (int)nbls, bad);
    FV_HIP(hipMemcpyAsync(hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
    throw_if_bad_solve_input(hbad);
    const SolveBlocks blk{sg.s, gp, dv, dd, dw, nrows, rows_per_unit, sums0.p, sums1.p};
    int cur = 0, niter = 0;
    while (niter < max_iter) {
        ++niter;
        normal(blk, dx[cur].as<cplx<double>>());
        update(blk, (const cplx<double> *)dx[cur].as<cplx<double>>(), dx[cur ^ 1].as<cplx<double>>(), niter & 1, dchange.as<double>(),
               dsolved.as<int>());
        cur ^= 1;
        FV_HIP(hipMemcpyAsync(change_out, dchange.p, sizeof(double) * (size_t)nunits, hipMemcpyDeviceToHost, sg.s));
        FV_HIP(hipStreamSynchronize(sg.s));  // (the one small synchronisation per iteration: the host decides)
        bool done = true;
        for (int64_t u = 0; u < nunits; ++u) done = done && change_out[u] < tol;
        if (done) break;
    }
    // the chi2 at the final iterate: the first scratch buffer holds the waves' partials
    chi2(blk, dx[cur].as<cplx<double>>());
    hipLaunchKernelGGL(k_gain_chi2_rows, dim3((unsigned)cdiv(nrows, 4)), dim3(256), 0, sg.s, (const double *)sums0.p, nrows, npart,
                       dchi2.as<double>());
    FV_HIP(hipMemcpyAsync(chi2_ft_out, dchi2.p, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(x, dx[cur].p, sizeof(cplx<double>) * nxu, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(solved_out, dsolved.p, sizeof(int) * nsu, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
    *niter_out = niter;
}

// Per-antenna gains: num (complex128) and den (float64) per (row, feed, antenna), k_gain_normal and k_gain_update.
template <typename T>
static void gain_solve_host(int device, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1, const int *ant2,
                            int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device,
                            const void *weights, int weights_on_device, void *gains, int max_iter, double tol, int *niter_out,
                            double *change_out, double *chi2_ft_out, int *solved_out) {
    const int ng = (tpol == 4 ? 2 : 1) * nant;
    const auto gather = [=](const SolveBlocks &b, const cplx<double> *g, bool chi2) {
        launch_gain_normal<T>(b.on, (const cplx<T> *)b.vis, (const cplx<T> *)b.data, (const T *)b.weights, g, b.gp, b.nrows,
                              b.rows_per_unit, tpol, chi2 ? nullptr : (cplx<double> *)b.sums0, chi2 ? nullptr : (double *)b.sums1,
                              chi2 ? (double *)b.sums0 : nullptr);
    };
    alternating_solve<T>(
        device, nfreqs, ntimes, nbls, nant, ant1, ant2, per_time, (int64_t)tpol * nbls, ng, ng, sizeof(cplx<double>) * ng,
        sizeof(double) * ng, ng, vis, vis_on_device, data, data_on_device, weights, weights_on_device, gains, max_iter, tol, niter_out,
        change_out, chi2_ft_out, solved_out, [=](const SolveBlocks &b, const cplx<double> *g) { gather(b, g, false); },
        [=](const SolveBlocks &b, const cplx<double> *g_old, cplx<double> *g_new, int odd, double *change, int *solved) {
            hipLaunchKernelGGL(k_gain_update, dim3((unsigned)(b.nrows / b.rows_per_unit)), dim3(256), 0, b.on,
                               (const cplx<double> *)b.sums0, (const double *)b.sums1, g_old, g_new, b.rows_per_unit, ng, odd, change,
                               solved);
        },
        [=](const SolveBlocks &b, const cplx<double> *g) { gather(b, g, true); });
}

// The redundant solve's two halves on host arrays (fv_redundant_vis_rows, fv_redundant_normal_rows): one row per unit.
// uvis_in: the groups' visibilities as given; the U-step copies them back with den, the gather writes num and den.
template <typename T>
static void redundant_rows_host(int device, bool vis_step, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                                const int *ant2, int ngroups, const int *group, const void *gains, void *uvis, const void *data,
                                const void *weights, void *num, double *den) {
    const int nfeed = tpol == 4 ? 2 : 1;
    const size_t ng = (size_t)nrows * nfeed * (size_t)nant, nu = (size_t)nrows * tpol * (size_t)ngroups;
    if (nrows == 0) return;
    if (nbls == 0) {  // (no sample: U keeps its values)
        if (!vis_step) std::memset(num, 0, sizeof(cplx<double>) * ng);
        std::memset(den, 0, sizeof(double) * (vis_step ? nu : ng));
        return;
    }
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nrows * (size_t)tpol * (size_t)nbls;
    GainPairs gp;
    gp.set(sg.s, nant, nbls, ant1, ant2);
    RedGroups rg;
    rg.set(sg.s, ngroups, nbls, group);
    DevBuf dd, dw, dgn, du, dnum, dden;
    const cplx<T> *d = to_device<cplx<T>>(sg.s, dd, data, n);
    const T *w = to_device<T>(sg.s, dw, weights, n);
    const cplx<double> *g = to_device<cplx<double>>(sg.s, dgn, gains, ng);
    cplx<double> *u = to_device<cplx<double>>(sg.s, du, uvis, nu);
    dden.reserve(sizeof(double) * (vis_step ? nu : ng));
    if (vis_step) {
        launch_red_vis<T>(sg.s, d, w, g, gp, rg, nrows, 1, tpol, u, dden.as<double>());
        FV_HIP(hipMemcpyAsync(uvis, du.p, sizeof(cplx<double>) * nu, hipMemcpyDeviceToHost, sg.s));
        FV_HIP(hipMemcpyAsync(den, dden.p, sizeof(double) * nu, hipMemcpyDeviceToHost, sg.s));
    } else {
        dnum.reserve(sizeof(cplx<double>) * ng);
        launch_red_normal<T>(sg.s, u, d, w, g, gp, rg, nrows, 1, tpol, dnum.as<cplx<double>>(), dden.as<double>(), nullptr);
        FV_HIP(hipMemcpyAsync(num, dnum.p, sizeof(cplx<double>) * ng, hipMemcpyDeviceToHost, sg.s));
        FV_HIP(hipMemcpyAsync(den, dden.p, sizeof(double) * ng, hipMemcpyDeviceToHost, sg.s));
    }
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

// Gains and one visibility per (row, pol, group): the U-step (k_red_vis) in front of the gain solve's gather with the
// groups' visibilities as its model, k_gain_update as it stands, and one more U-step at the returned gains before chi2.
// U and its den live in buffers of this call; they come to the host once, at the end.
template <typename T>
static void redundant_solve_host(int device, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                                 const int *ant2, int ngroups, const int *group, int per_time, const void *data, int data_on_device,
                                 const void *weights, int weights_on_device, void *gains, void *uvis_out, int max_iter, double tol,
                                 int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, int *vis_solved_out) {
    const int ng = (tpol == 4 ? 2 : 1) * nant;
    const int64_t nrows = (int64_t)nfreqs * ntimes;
    const size_t nu = (size_t)nrows * tpol * (size_t)ngroups;
    RedGroups rg;
    DevBuf du, dden;
    if (nrows > 0 && nbls > 0) {
        FV_HIP(hipSetDevice(device));
        StreamGuard sg;
        rg.set(sg.s, ngroups, nbls, group);
        du.reserve(sizeof(cplx<double>) * nu);
        dden.reserve(sizeof(double) * nu);
        FV_HIP(hipMemsetAsync(du.p, 0, sizeof(cplx<double>) * nu, sg.s));  // the start: U = 0
        FV_HIP(hipStreamSynchronize(sg.s));
    }
    cplx<double> *u = du.as<cplx<double>>();
    double *uden = dden.as<double>();
    const RedGroups &groups = rg;
    const auto step = [=, &groups](const SolveBlocks &b, const cplx<double> *g, bool chi2) {
        launch_red_vis<T>(b.on, (const cplx<T> *)b.data, (const T *)b.weights, g, b.gp, groups, b.nrows, b.rows_per_unit, tpol, u, uden);
        launch_red_normal<T>(b.on, u, (const cplx<T> *)b.data, (const T *)b.weights, g, b.gp, groups, b.nrows, b.rows_per_unit, tpol,
                             chi2 ? nullptr : (cplx<double> *)b.sums0, chi2 ? nullptr : (double *)b.sums1,
                             chi2 ? (double *)b.sums0 : nullptr);
    };
    alternating_solve<T>(
        device, nfreqs, ntimes, nbls, nant, ant1, ant2, per_time, (int64_t)tpol * nbls, ng, ng, sizeof(cplx<double>) * ng,
        sizeof(double) * ng, ng, nullptr, 0, data, data_on_device, weights, weights_on_device, gains, max_iter, tol, niter_out,
        change_out, chi2_ft_out, solved_out, [=](const SolveBlocks &b, const cplx<double> *g) { step(b, g, false); },
        [=](const SolveBlocks &b, const cplx<double> *g_old, cplx<double> *g_new, int odd, double *change, int *solved) {
            hipLaunchKernelGGL(k_gain_update, dim3((unsigned)(b.nrows / b.rows_per_unit)), dim3(256), 0, b.on,
                               (const cplx<double> *)b.sums0, (const double *)b.sums1, g_old, g_new, b.rows_per_unit, ng, odd, change,
                               solved);
        },
        [=](const SolveBlocks &b, const cplx<double> *g) { step(b, g, true); });
    if (nrows == 0) return;
    if (nbls == 0) {  // (the start: U = 0, nothing solved)
        std::memset(uvis_out, 0, sizeof(cplx<double>) * nu);
        std::fill(vis_solved_out, vis_solved_out + nu, 0);
        return;
    }
    std::vector<double> hden(nu);  // (the solve has ended and synchronised its stream: U and den are complete)
    FV_HIP(hipMemcpy(uvis_out, du.p, sizeof(cplx<double>) * nu, hipMemcpyDeviceToHost));
    FV_HIP(hipMemcpy(hden.data(), dden.p, sizeof(double) * nu, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nu; ++i) vis_solved_out[i] = hden[i] > 0.0 ? 1 : 0;
}

// Firstcal, stage 1 (k_firstcal_products, k_firstcal_delay): a device block is used where it lies, a host block is staged
// once; the twiddles exp(-2 pi i j / ND) are built here in fp64; the five outputs, (nfeed, npairs), come back at the end.
template <typename T>
static void firstcal_pair_delays_host(int device, int nfreqs, int ntimes, int64_t nbls, int tpol, int npairs, const int *pair1,
                                      const int *pair2, const int *ant1, const int *ant2, const void *data,
                                      int data_on_device, const void *weights, int weights_on_device, int pad, int *peak_bin_out,
                                      double *delay_bins_out, double *power_out, double *total_out, int *used_out) {
    const size_t nrows = (size_t)(tpol == 4 ? 2 : 1) * (size_t)npairs;
    if (nrows == 0) return;
    std::fill(peak_bin_out, peak_bin_out + nrows, 0);
    std::fill(delay_bins_out, delay_bins_out + nrows, 0.0);
    std::fill(power_out, power_out + nrows, 0.0);
    std::fill(total_out, total_out + nrows, 0.0);
    std::fill(used_out, used_out + nrows, 0);
    if (nfreqs == 0 || ntimes == 0 || nbls == 0) return;  // (no sample: no pair is used)
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nfreqs * (size_t)ntimes * (size_t)tpol * (size_t)nbls;
    const int nd = pad * nfreqs;
    std::vector<cplx<double>> tw((size_t)nd);
    for (int j = 0; j < nd; ++j) tw[j] = {std::cos(2.0 * M_PI * (double)j / nd), -std::sin(2.0 * M_PI * (double)j / nd)};
    DevBuf sd, sw, da1, da2, dp1, dp2, dtw, dz, dbin, dx, dpow, dtot, dused;
    const cplx<T> *dd = data_on_device ? static_cast<const cplx<T> *>(data) : to_device<cplx<T>>(sg.s, sd, data, n);
    const T *dw = weights_on_device ? static_cast<const T *>(weights) : to_device<T>(sg.s, sw, weights, n);
    const int *a1 = to_device<int>(sg.s, da1, ant1, (size_t)nbls), *a2 = to_device<int>(sg.s, da2, ant2, (size_t)nbls);
    const int *p1 = to_device<int>(sg.s, dp1, pair1, (size_t)npairs), *p2 = to_device<int>(sg.s, dp2, pair2, (size_t)npairs);
    const cplx<double> *dt = to_device<cplx<double>>(sg.s, dtw, tw.data(), (size_t)nd);
    dz.reserve(sizeof(cplx<double>) * nrows * (size_t)nfreqs);
    dbin.reserve(sizeof(int) * nrows);
    dx.reserve(sizeof(double) * nrows);
    dpow.reserve(sizeof(double) * nrows);
    dtot.reserve(sizeof(double) * nrows);
    dused.reserve(sizeof(int) * nrows);
    launch_firstcal_delays<T>(sg.s, dd, dw, a1, a2, (int)nbls, p1, p2, nfreqs, ntimes, tpol, npairs, dt, nd, dz.as<cplx<double>>(), dbin.as<int>(),
                              dx.as<double>(), dpow.as<double>(), dtot.as<double>(), dused.as<int>());
    FV_HIP(hipMemcpyAsync(peak_bin_out, dbin.p, sizeof(int) * nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(delay_bins_out, dx.p, sizeof(double) * nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(power_out, dpow.p, sizeof(double) * nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(total_out, dtot.p, sizeof(double) * nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(used_out, dused.p, sizeof(int) * nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

// Firstcal, stage 2: the block derotated by the delay model into a buffer of this call (k_firstcal_derotate; the caller's
// data are read only), then the redundant solve on it with the whole block as one unit -- redundant_solve_host with one
// "frequency" of nfreqs ntimes "times": the (nfreqs, ntimes) block is contiguous, U and chi2 stay per row.
template <typename T>
static void firstcal_offsets_host(int device, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                                  const int *ant2, int ngroups, const int *group, const double *slopes, const void *data,
                                  int data_on_device, const void *weights, int weights_on_device, void *offsets, void *uvis_out,
                                  int max_iter, double tol, int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out,
                                  int *vis_solved_out) {
    const int nfeed = tpol == 4 ? 2 : 1;
    const size_t n = (size_t)nfreqs * (size_t)ntimes * (size_t)tpol * (size_t)nbls;
    DevBuf sd, sw, ds, rotated;
    const void *dw = weights;
    if (n > 0) {
        FV_HIP(hipSetDevice(device));
        StreamGuard sg;
        GainPairs gp;
        gp.set(sg.s, nant, nbls, ant1, ant2);
        const cplx<T> *dd = data_on_device ? static_cast<const cplx<T> *>(data) : to_device<cplx<T>>(sg.s, sd, data, n);
        dw = weights_on_device ? weights : to_device<T>(sg.s, sw, weights, n);  // (null stays null)
        const double *dsl = to_device<double>(sg.s, ds, slopes, (size_t)nfeed * (size_t)nant);
        rotated.reserve(sizeof(cplx<T>) * n);
        hipLaunchKernelGGL(k_firstcal_derotate<T>, dim3((unsigned)std::min<int64_t>(cdiv((int64_t)n, 256), 65535)), dim3(256), 0, sg.s,
                           dd, static_cast<const T *>(dw), gp.d_ant1.as<int>(), gp.d_ant2.as<int>(), dsl, (int64_t)n, nfreqs, ntimes,
                           (int)nbls, tpol, nant, rotated.as<cplx<T>>());
        FV_HIP(hipStreamSynchronize(sg.s));  // (the solve runs on a stream of its own)
        FV_HIP(hipGetLastError());
    }
    redundant_solve_host<T>(device, nfreqs > 0 ? 1 : 0, nfreqs * ntimes, nbls, tpol, nant, ant1, ant2, ngroups, group, 0, rotated.p, 1,
                            dw, weights ? 1 : 0, offsets, uvis_out, max_iter, tol, niter_out, change_out, chi2_ft_out, solved_out,
                            vis_solved_out);
}

// Abscal (k_abscal_products, k_abscal_search, k_abscal_peak, k_abscal_refine, k_abscal_chi2): the groups' in-plane
// coordinates split into x1, x2 (x2 = 0 for a line), the search's axes (the runs along 1 when n2 == 1) and its step
// factors exp(i h_b x_b), built here in fp64.
struct AbscalCoords {
    DevBuf d1, d2, dstep;
    fv::AbscalGrid ag{};
    void set(hipStream_t s, int ngroups, const double *coords, int ndim, int n1, int n2, double h1, double h2) {
        std::vector<double> x1((size_t)ngroups), x2((size_t)ngroups, 0.0);
        for (int g = 0; g < ngroups; ++g) {
            x1[g] = coords[(size_t)g * ndim];
            if (ndim == 2) x2[g] = coords[(size_t)g * 2 + 1];
        }
        const bool swap = n2 == 1;
        const double hb = swap ? h1 : h2;
        std::vector<cplx<double>> step((size_t)ngroups);
        for (int g = 0; g < ngroups; ++g) {
            const double t = hb * (swap ? x1[g] : x2[g]);
            step[g] = {std::cos(t), std::sin(t)};
        }
        d1.reserve(sizeof(double) * (size_t)ngroups);
        d2.reserve(sizeof(double) * (size_t)ngroups);
        dstep.reserve(sizeof(cplx<double>) * (size_t)ngroups);
        // (pageable host memory: the copies have left the vectors when the calls return)
        FV_HIP(hipMemcpyAsync(d1.p, x1.data(), sizeof(double) * (size_t)ngroups, hipMemcpyHostToDevice, s));
        FV_HIP(hipMemcpyAsync(d2.p, x2.data(), sizeof(double) * (size_t)ngroups, hipMemcpyHostToDevice, s));
        FV_HIP(hipMemcpyAsync(dstep.p, step.data(), sizeof(cplx<double>) * (size_t)ngroups, hipMemcpyHostToDevice, s));
        FV_HIP(hipStreamSynchronize(s));
        const double *a = d1.as<double>(), *b = d2.as<double>();
        ag = {a, b, swap ? b : a, swap ? a : b, dstep.as<cplx<double>>(), ndim, n1, n2, swap ? n2 : n1, swap ? n1 : n2,
              h1, h2, swap ? h2 : h1, hb};
    }
};
template <typename T>
static void abscal_slopes_host(int device, int nfreqs, int ntimes, int tpol, int ngroups, int per_time, const void *uvis,
                               int uvis_on_device, const void *model, int model_on_device, const void *gweights,
                               int gweights_on_device, const double *coords, int ndim, int n1, int n2, double h1, double h2, int refine,
                               int *peak_out, double *slopes_out, double *amp_out, double *power_out, double *unorm_out,
                               double *mnorm_out, int *used_out, double *chi2_ft_out) {
    const int nfeed = tpol == 4 ? 2 : 1, nunits = per_time ? nfreqs * ntimes : nfreqs, nrows = nunits * nfeed;
    const int64_t nft = (int64_t)nfreqs * ntimes;
    std::fill(peak_out, peak_out + 2 * (size_t)nrows, 0);  // the neutral result
    std::fill(slopes_out, slopes_out + 2 * (size_t)nrows, 0.0);
    std::fill(amp_out, amp_out + nrows, 1.0);
    std::fill(power_out, power_out + nrows, 0.0);
    std::fill(unorm_out, unorm_out + nrows, 0.0);
    std::fill(mnorm_out, mnorm_out + nrows, 0.0);
    std::fill(used_out, used_out + nrows, 0);
    std::fill(chi2_ft_out, chi2_ft_out + nft, 0.0);
    if (nft == 0 || ngroups == 0) return;
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nft * (size_t)tpol * (size_t)ngroups, nrg = (size_t)nrows * (size_t)ngroups;
    DevBuf su, sm, sw, dc, dng, dpg, dcnt, dbad, dtv, dti, dpi, dpeak, dsl, damp, dpow, dun, dmn, dused, drows;
    const cplx<double> *du = uvis_on_device ? static_cast<const cplx<double> *>(uvis) : to_device<cplx<double>>(sg.s, su, uvis, n);
    const cplx<T> *dm = model_on_device ? static_cast<const cplx<T> *>(model) : to_device<cplx<T>>(sg.s, sm, model, n);
    const double *dw = gweights_on_device ? static_cast<const double *>(gweights) : to_device<double>(sg.s, sw, gweights, n);
    AbscalCoords co;
    co.set(sg.s, ngroups, coords, ndim, n1, n2, h1, h2);
    const size_t ntiles = (size_t)abscal_tiles(co.ag);
    dc.reserve(sizeof(cplx<double>) * nrg);
    dng.reserve(sizeof(double) * nrg);
    dpg.reserve(sizeof(double) * nrg);
    dcnt.reserve(sizeof(int) * nrg);
    dbad.reserve(16);
    dtv.reserve(sizeof(double) * (size_t)nrows * ntiles);
    dti.reserve(sizeof(int) * (size_t)nrows * ntiles);
    dpi.reserve(sizeof(int) * (size_t)nrows);
    dpeak.reserve(sizeof(int) * 2 * (size_t)nrows);
    dsl.reserve(sizeof(double) * 2 * (size_t)nrows);
    for (DevBuf *b : {&damp, &dpow, &dun, &dmn}) b->reserve(sizeof(double) * (size_t)nrows);
    dused.reserve(sizeof(int) * (size_t)nrows);
    int hbad[3] = {0, 0, 0};
    FV_HIP(hipMemsetAsync(dbad.p, 0, sizeof(hbad), sg.s));
    launch_abscal_fit<T>(sg.s, du, dm, dw, co.ag, nunits, ntimes, tpol, ngroups, per_time, refine, dc.as<cplx<double>>(), dng.as<double>(),
                         dpg.as<double>(), dcnt.as<int>(), dbad.as<int>(), dtv.as<double>(), dti.as<int>(), dpi.as<int>(), dpeak.as<int>(),
                         dsl.as<double>(), damp.as<double>(), dpow.as<double>(), dun.as<double>(), dmn.as<double>(), dused.as<int>());
    const int nblk = (int)cdiv((int64_t)nfeed * ngroups, 256);
    drows.reserve(sizeof(double) * (size_t)nft * ((size_t)nblk + 1));
    double *partials = drows.as<double>(), *sums = partials + (size_t)nft * nblk;
    hipLaunchKernelGGL(k_abscal_chi2<T>, dim3((unsigned)nblk, (unsigned)std::min<int64_t>(nft, 65535)), dim3(256), 0, sg.s, du, dm, dw,
                       co.ag.x1, co.ag.x2, (const double *)damp.as<double>(), (const double *)dsl.as<double>(), nft, ntimes, tpol, ngroups,
                       per_time, partials);
    hipLaunchKernelGGL(k_chi2_rows_reduce, dim3((unsigned)cdiv(nft, 256)), dim3(256), 0, sg.s, (const double *)partials, nft, nblk, sums);
    std::vector<int> hpeak(2 * (size_t)nrows), hused((size_t)nrows);
    std::vector<double> hsl(2 * (size_t)nrows), hamp((size_t)nrows), hpow((size_t)nrows), hun((size_t)nrows), hmn((size_t)nrows),
        hchi2((size_t)nft);
    FV_HIP(hipMemcpyAsync(hbad, dbad.p, sizeof(hbad), hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hpeak.data(), dpeak.p, sizeof(int) * 2 * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hsl.data(), dsl.p, sizeof(double) * 2 * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hamp.data(), damp.p, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hpow.data(), dpow.p, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hun.data(), dun.p, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hmn.data(), dmn.p, sizeof(double) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hused.data(), dused.p, sizeof(int) * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(hchi2.data(), sums, sizeof(double) * (size_t)nft, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
    throw_if_bad_solve_input(hbad);  // (before any output is written: a failed call leaves the neutral result)
    std::copy(hpeak.begin(), hpeak.end(), peak_out);
    std::copy(hsl.begin(), hsl.end(), slopes_out);
    std::copy(hamp.begin(), hamp.end(), amp_out);
    std::copy(hpow.begin(), hpow.end(), power_out);
    std::copy(hun.begin(), hun.end(), unorm_out);
    std::copy(hmn.begin(), hmn.end(), mnorm_out);
    std::copy(hused.begin(), hused.end(), used_out);
    std::copy(hchi2.begin(), hchi2.end(), chi2_ft_out);
}
static void abscal_evaluate_host(int device, int nrows, int ngroups, const void *c, const double *coords, int ndim, const double *slopes,
                                 double *out) {
    std::fill(out, out + 6 * (size_t)nrows, 0.0);
    if (nrows == 0 || ngroups == 0) return;
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    DevBuf dc, dsl, dout;
    AbscalCoords co;
    co.set(sg.s, ngroups, coords, ndim, 1, 1, 1.0, 1.0);
    const cplx<double> *pc = to_device<cplx<double>>(sg.s, dc, c, (size_t)nrows * (size_t)ngroups);
    const double *ps = to_device<double>(sg.s, dsl, slopes, 2 * (size_t)nrows);
    dout.reserve(sizeof(double) * 6 * (size_t)nrows);
    const int in_lds = abscal_in_lds(ngroups);
    hipLaunchKernelGGL(k_abscal_evaluate, dim3((unsigned)cdiv(nrows, 4)), dim3(256), in_lds ? sizeof(double) * 10 * (size_t)ngroups : 0, sg.s,
                       pc, co.ag.x1, co.ag.x2, ps, nrows, ngroups, in_lds, dout.as<double>());
    FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * 6 * (size_t)nrows, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

template <typename T>
static void jones_normal_rows_host(int device, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                                   const void *jones, const void *vis, const void *data, const void *weights, double *A_out,
                                   void *b_out) {
    const size_t nj = (size_t)nrows * 4 * (size_t)nant;
    if (nrows == 0) return;
    if (nbls == 0) {
        std::memset(A_out, 0, sizeof(double) * 2 * nj);
        std::memset(b_out, 0, sizeof(cplx<double>) * nj);
        return;
    }
    FV_HIP(hipSetDevice(device));
    StreamGuard sg;
    const size_t n = (size_t)nrows * 4 * (size_t)nbls;
    GainPairs gp;
    gp.set(sg.s, nant, nbls, ant1, ant2);
    DevBuf dv, dd, dw, djn, dA, db;
    dA.reserve(sizeof(double) * 2 * nj);
    db.reserve(sizeof(cplx<double>) * nj);
    launch_jones_normal<T>(sg.s, to_device<cplx<T>>(sg.s, dv, vis, n), to_device<cplx<T>>(sg.s, dd, data, n),
                           to_device<T>(sg.s, dw, weights, n), to_device<cplx<double>>(sg.s, djn, jones, nj), gp, nrows, 1,
                           dA.as<double>(), db.as<cplx<double>>(), nullptr);
    FV_HIP(hipMemcpyAsync(A_out, dA.p, sizeof(double) * 2 * nj, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipMemcpyAsync(b_out, db.p, sizeof(cplx<double>) * nj, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

// 2 x 2 matrices: A (8 float64) and b (4 complex128) per (row, antenna), k_jones_normal and k_jones_update.
template <typename T>
static void jones_solve_host(int device, int nfreqs, int ntimes, int64_t nbls, int nant, const int *ant1, const int *ant2,
                             int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device,
                             const void *weights, int weights_on_device, void *jones, int max_iter, double tol, int *niter_out,
                             double *change_out, double *chi2_ft_out, int *solved_out) {
    const auto gather = [=](const SolveBlocks &b, const cplx<double> *j, bool chi2) {
        launch_jones_normal<T>(b.on, (const cplx<T> *)b.vis, (const cplx<T> *)b.data, (const T *)b.weights, j, b.gp, b.nrows,
                               b.rows_per_unit, chi2 ? nullptr : (double *)b.sums0, chi2 ? nullptr : (cplx<double> *)b.sums1,
                               chi2 ? (double *)b.sums0 : nullptr);
    };
    alternating_solve<T>(
        device, nfreqs, ntimes, nbls, nant, ant1, ant2, per_time, 4 * nbls, 4 * nant, 2 * nant, sizeof(double) * 8 * nant,
        sizeof(cplx<double>) * 4 * nant, nant, vis, vis_on_device, data, data_on_device, weights, weights_on_device, jones, max_iter, tol,
        niter_out, change_out, chi2_ft_out, solved_out, [=](const SolveBlocks &b, const cplx<double> *j) { gather(b, j, false); },
        [=](const SolveBlocks &b, const cplx<double> *j_old, cplx<double> *j_new, int odd, double *change, int *solved) {
            hipLaunchKernelGGL(k_jones_update, dim3((unsigned)(b.nrows / b.rows_per_unit)), dim3(256), 0, b.on, (const double *)b.sums0,
                               (const cplx<double> *)b.sums1, j_old, j_new, b.rows_per_unit, nant, odd, change, solved);
        },
        [=](const SolveBlocks &b, const cplx<double> *j) { gather(b, j, true); });
}

template <typename T>
static void inplace_rot_host(int device, const double *rot, void *b, int64_t n) {
    FV_REQUIRE(rot && n >= 0 && (b || n == 0), "bad inplace_rot arrays");
    FV_HIP(hipSetDevice(device));
    if (n == 0) return;
    StreamGuard sg;
    DevBuf db;
    db.reserve(sizeof(T) * 3 * n);
    Rot9 r;
    std::memcpy(r.m, rot, sizeof(r.m));
    FV_HIP(hipMemcpyAsync(db.p, b, sizeof(T) * 3 * n, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(k_inplace_rot<T>, dim3(cdiv(n, 256)), dim3(256), 0, sg.s, r, db.as<T>(), n);
    FV_HIP(hipMemcpyAsync(b, db.p, sizeof(T) * 3 * n, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

template <typename T>
static void astrom_topo_host(int device, const double *astrom, int64_t n, const void *eq, void *out) {
    FV_REQUIRE(astrom && n >= 0 && ((eq && out) || n == 0), "bad astrom_topo arrays");
    FV_HIP(hipSetDevice(device));
    if (n == 0) return;
    Astrom a;
    std::memcpy(&a, astrom, sizeof(a));
    FV_REQUIRE(a.em > 0 && a.bm1 > 0, "astrometry context: em and bm1 must be positive");
    StreamGuard sg;
    DevBuf din, dout;
    din.reserve(sizeof(T) * 3 * n);
    dout.reserve(sizeof(T) * 3 * n);
    FV_HIP(hipMemcpyAsync(din.p, eq, sizeof(T) * 3 * n, hipMemcpyHostToDevice, sg.s));
    hipLaunchKernelGGL(k_astrom_topo<T>, dim3(cdiv(n, 256)), dim3(256), 0, sg.s, n, n, (int64_t)0, din.as<T>(), a, dout.as<T>());
    FV_HIP(hipMemcpyAsync(out, dout.p, sizeof(T) * 3 * n, hipMemcpyDeviceToHost, sg.s));
    FV_HIP(hipStreamSynchronize(sg.s));
    FV_HIP(hipGetLastError());
}

}  // namespace fv

using namespace fv;

struct fv_sim {
    std::unique_ptr<SimBase> impl;
    int precision;
};

extern "C" {

int fv_version(void) { return 100; /* 0.1.0 */ }
int fv_release_workspaces(void) {
    return guarded([&] {  // every thread's: call while no fv_nufft3 / fv_nudft3_direct is in flight
        workspace_slot<double>() = nullptr;
        workspace_slot<float>() = nullptr;
        WorkspaceRegistry<double>::get().drain();
        WorkspaceRegistry<float>::get().drain();
    });
}
int fv_device_bytes(int64_t *bytes) {
    if (bytes) *bytes = (int64_t)fv::dev_bytes_held().load();
    return bytes ? 0 : 1;
}

int fv_device_bytes_on(int device, int64_t *bytes) {
    if (bytes) *bytes = (int64_t)fv::dev_bytes_on(device).load();
    return bytes ? 0 : 1;
}

int fv_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes) {
    return guarded([&] {
        FV_REQUIRE(free_bytes && total_bytes, "null output");
        FV_HIP(hipSetDevice(device));
        size_t f = 0, t = 0;
        FV_HIP(hipMemGetInfo(&f, &t));
        *free_bytes = (int64_t)f;
        *total_bytes = (int64_t)t;
    });
}

int fv_device_count(int *count) {
    return guarded([&] {
        FV_REQUIRE(count, "null count");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            n = 0;
        }
        *count = n;
    });
}

const char *fv_last_error(void) { return g_last_error.c_str(); }

int fv_nufft3(int device, int precision, int dim, int64_t M, const void *x, const void *y,
              const void *z, const void *c, int ntrans, int64_t N, const void *s, const void *t,
              const void *u, double eps, double upsampfac, void *out) {
    return guarded(precision, [&](auto real) {
        const void *xs[3] = {x, y, z}, *ss[3] = {s, t, u};
        nufft3_host<decltype(real)>(device, dim, M, xs, c, ntrans, N, ss, eps, upsampfac, out, false);
    });
}

int fv_nudft3_direct(int device, int precision, int dim, int64_t M, const void *x, const void *y,
                     const void *z, const void *c, int ntrans, int64_t N, const void *s,
                     const void *t, const void *u, void *out) {
    return guarded(precision, [&](auto real) {
        const void *xs[3] = {x, y, z}, *ss[3] = {s, t, u};
        nufft3_host<decltype(real)>(device, dim, M, xs, c, ntrans, N, ss, 0, 2.0, out, true);
    });
}

int fv_beam_eval(int device, int precision, int polarized, int kind, double diameter,
                 int nfreq_tab, int nza, int naz, double za_max, const void *table, int order,
                 int freq_index, double freq, int64_t n, const void *az, const void *za, void *out) {
    return guarded(precision, [&](auto real) {
        beam_eval_host<decltype(real)>(device, polarized, kind, diameter, nfreq_tab, nza, naz, za_max, table, order, freq_index,
                                       freq, n, az, za, out);
    });
}

int fv_apparent_coherency(int device, int precision, int variant, int64_t n, const void *beam_i,
                          const void *beam_j, const void *flux, void *out) {
    return guarded(precision, [&](auto real) { coherency_host<decltype(real)>(device, variant, n, beam_i, beam_j, flux, out); });
}

int fv_residual_chi2(int device, int precision, int64_t nrows, int64_t row_len, void *vis, const void *data,
                     const void *weights, double *chi2_rows) {
    return guarded(precision, [&](auto real) {
        FV_REQUIRE(nrows >= 0 && row_len >= 0, "fv_residual_chi2: negative shape");
        FV_REQUIRE((nrows == 0 || row_len == 0 || (vis && data)) && (nrows == 0 || chi2_rows), "fv_residual_chi2: null vis, data or chi2_rows");
        FV_HIP(hipSetDevice(device));  // (asked of an empty call too)
        residual_rows_host<decltype(real)>(device, nrows, row_len, vis, data, weights, chi2_rows);
    });
}

int fv_gain_residual_chi2(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                          const int *ant2, const void *gains, void *vis, const void *data, const void *weights,
                          double *chi2_rows, void *ggains) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_gain_residual_chi2: tpol must be 1 or 4");
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_gain_residual_chi2: negative shape");
        FV_REQUIRE(nant >= 1, "fv_gain_residual_chi2: nant must be positive");
        FV_REQUIRE(gains || nrows == 0, "fv_gain_residual_chi2: null gains");
        FV_REQUIRE((nrows == 0 || nbls == 0 || (vis && data && ant1 && ant2)) && (nrows == 0 || chi2_rows),
                   "fv_gain_residual_chi2: null pairs, vis, data or chi2_rows");
        if (nrows > 0) require_pairs("fv_gain_residual_chi2", nbls, nant, ant1, ant2);
        residual_rows_host<decltype(real)>(device, nrows, tpol * nbls, vis, data, weights, chi2_rows,
                                           {Cal::Gains, tpol, nant, nbls, ant1, ant2, gains, nullptr, ggains});
    });
}

int fv_jones_residual_chi2(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                           const void *jones, void *vis, const void *data, const void *weights, double *chi2_rows,
                           void *gjones) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_jones_residual_chi2: negative shape");
        FV_REQUIRE(nant >= 1, "fv_jones_residual_chi2: nant must be positive");
        FV_REQUIRE(jones || nrows == 0, "fv_jones_residual_chi2: null jones");
        FV_REQUIRE((nrows == 0 || nbls == 0 || (vis && data && ant1 && ant2)) && (nrows == 0 || chi2_rows),
                   "fv_jones_residual_chi2: null pairs, vis, data or chi2_rows");
        if (nrows > 0) require_pairs("fv_jones_residual_chi2", nbls, nant, ant1, ant2);
        residual_rows_host<decltype(real)>(device, nrows, 4 * nbls, vis, data, weights, chi2_rows,
                                           {Cal::Jones, 4, nant, nbls, ant1, ant2, jones, nullptr, gjones});
    });
}

int fv_gain_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, const void *gains, const void *vis, const void *data, const void *weights, void *num,
                        double *den) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_gain_normal_rows: tpol must be 1 or 4");
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_gain_normal_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_gain_normal_rows: nant must be positive");
        FV_REQUIRE(nrows == 0 || (gains && num && den), "fv_gain_normal_rows: null gains, num or den");
        FV_REQUIRE(nrows == 0 || nbls == 0 || (vis && data && ant1 && ant2), "fv_gain_normal_rows: null pairs, vis or data");
        if (nrows > 0) require_pairs("fv_gain_normal_rows", nbls, nant, ant1, ant2);
        gain_normal_rows_host<decltype(real)>(device, nrows, nbls, tpol, nant, ant1, ant2, gains, vis, data, weights, num, den);
    });
}

int fv_gain_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                  const int *ant2, int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device,
                  const void *weights, int weights_on_device, void *gains, int max_iter, double tol, int *niter_out,
                  double *change_out, double *chi2_ft_out, int *solved_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_gain_solve: tpol must be 1 or 4");
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_gain_solve: negative shape");
        FV_REQUIRE(nant >= 1, "fv_gain_solve: nant must be positive");
        FV_REQUIRE(max_iter >= 1, "fv_gain_solve: max_iter must be positive");
        FV_REQUIRE(tol >= 0.0, "fv_gain_solve: tol must be non-negative");  // (a NaN fails the comparison)
        FV_REQUIRE(((per_time | vis_on_device | data_on_device | weights_on_device) & ~1) == 0,
                   "fv_gain_solve: per_time and the on_device flags must be 0 or 1");
        FV_REQUIRE(niter_out, "fv_gain_solve: null niter_out");
        const bool empty = nfreqs == 0 || ntimes == 0;
        FV_REQUIRE(empty || (gains && change_out && chi2_ft_out && solved_out),
                   "fv_gain_solve: null gains, change_out, chi2_ft_out or solved_out");
        FV_REQUIRE(empty || nbls == 0 || (vis && data && ant1 && ant2), "fv_gain_solve: null pairs, vis or data");
        if (!empty) require_pairs("fv_gain_solve", nbls, nant, ant1, ant2);
        gain_solve_host<decltype(real)>(device, nfreqs, ntimes, nbls, tpol, nant, ant1, ant2, per_time, vis, vis_on_device, data,
                                        data_on_device, weights, weights_on_device, gains, max_iter, tol, niter_out, change_out,
                                        chi2_ft_out, solved_out);
    });
}

static void require_groups(const char *entry, int64_t nbls, int ngroups, const int *group) {
    for (int64_t k = 0; k < nbls; ++k)
        FV_REQUIRE(group[k] >= 0 && group[k] < ngroups, std::string(entry) + ": group index outside [0, ngroups)");
}

int fv_redundant_vis_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                          const int *ant2, int ngroups, const int *group, const void *gains, const void *data,
                          const void *weights, void *uvis, double *den) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_redundant_vis_rows: tpol must be 1 or 4");
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_redundant_vis_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_redundant_vis_rows: nant must be positive");
        FV_REQUIRE(ngroups >= 1, "fv_redundant_vis_rows: ngroups must be positive");
        FV_REQUIRE(nrows == 0 || (gains && uvis && den), "fv_redundant_vis_rows: null gains, uvis or den");
        FV_REQUIRE(nrows == 0 || nbls == 0 || (data && ant1 && ant2 && group), "fv_redundant_vis_rows: null pairs, group or data");
        if (nrows > 0) require_pairs("fv_redundant_vis_rows", nbls, nant, ant1, ant2);
        if (nrows > 0) require_groups("fv_redundant_vis_rows", nbls, ngroups, group);
        redundant_rows_host<decltype(real)>(device, true, nrows, nbls, tpol, nant, ant1, ant2, ngroups, group, gains, uvis, data,
                                            weights, nullptr, den);
    });
}

int fv_redundant_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                             const int *ant2, int ngroups, const int *group, const void *gains, const void *uvis,
                             const void *data, const void *weights, void *num, double *den) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_redundant_normal_rows: tpol must be 1 or 4");
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_redundant_normal_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_redundant_normal_rows: nant must be positive");
        FV_REQUIRE(ngroups >= 1, "fv_redundant_normal_rows: ngroups must be positive");
        FV_REQUIRE(nrows == 0 || (gains && num && den), "fv_redundant_normal_rows: null gains, num or den");
        FV_REQUIRE(nrows == 0 || nbls == 0 || (uvis && data && ant1 && ant2 && group),
                   "fv_redundant_normal_rows: null pairs, group, uvis or data");
        if (nrows > 0) require_pairs("fv_redundant_normal_rows", nbls, nant, ant1, ant2);
        if (nrows > 0) require_groups("fv_redundant_normal_rows", nbls, ngroups, group);
        redundant_rows_host<decltype(real)>(device, false, nrows, nbls, tpol, nant, ant1, ant2, ngroups, group, gains,
                                            const_cast<void *>(uvis), data, weights, num, den);
    });
}

int fv_redundant_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                       const int *ant2, int ngroups, const int *group, int per_time, const void *data, int data_on_device,
                       const void *weights, int weights_on_device, void *gains, void *uvis_out, int max_iter, double tol,
                       int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, int *vis_solved_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_redundant_solve: tpol must be 1 or 4");
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_redundant_solve: negative shape");
        FV_REQUIRE(nant >= 1, "fv_redundant_solve: nant must be positive");
        FV_REQUIRE(ngroups >= 1, "fv_redundant_solve: ngroups must be positive");
        FV_REQUIRE(max_iter >= 1, "fv_redundant_solve: max_iter must be positive");
        FV_REQUIRE(tol >= 0.0, "fv_redundant_solve: tol must be non-negative");  // (a NaN fails the comparison)
        FV_REQUIRE(((per_time | data_on_device | weights_on_device) & ~1) == 0,
                   "fv_redundant_solve: per_time and the on_device flags must be 0 or 1");
        FV_REQUIRE(niter_out, "fv_redundant_solve: null niter_out");
        const bool empty = nfreqs == 0 || ntimes == 0;
        FV_REQUIRE(empty || (gains && uvis_out && change_out && chi2_ft_out && solved_out && vis_solved_out),
                   "fv_redundant_solve: null gains, uvis_out, change_out, chi2_ft_out, solved_out or vis_solved_out");
        FV_REQUIRE(empty || nbls == 0 || (data && ant1 && ant2 && group), "fv_redundant_solve: null pairs, group or data");
        if (!empty) require_pairs("fv_redundant_solve", nbls, nant, ant1, ant2);
        if (!empty) require_groups("fv_redundant_solve", nbls, ngroups, group);
        redundant_solve_host<decltype(real)>(device, nfreqs, ntimes, nbls, tpol, nant, ant1, ant2, ngroups, group, per_time, data,
                                             data_on_device, weights, weights_on_device, gains, uvis_out, max_iter, tol, niter_out,
                                             change_out, chi2_ft_out, solved_out, vis_solved_out);
    });
}

int fv_firstcal_pair_delays(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int npairs, const int *pair1,
                            const int *pair2, const int *ant1, const int *ant2, const void *data, int data_on_device,
                            const void *weights, int weights_on_device, int pad, int *peak_bin_out, double *delay_bins_out,
                            double *power_out, double *total_out, int *used_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_firstcal_pair_delays: tpol must be 1 or 4");
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29) && npairs >= 0 && npairs < (1 << 29),
                   "fv_firstcal_pair_delays: negative shape");
        FV_REQUIRE(pad >= 1 && (int64_t)pad * nfreqs < ((int64_t)1 << 20), "fv_firstcal_pair_delays: pad must be positive and pad nfreqs below 2^20");
        FV_REQUIRE(((data_on_device | weights_on_device) & ~1) == 0, "fv_firstcal_pair_delays: the on_device flags must be 0 or 1");
        FV_REQUIRE(npairs == 0 || (peak_bin_out && delay_bins_out && power_out && total_out && used_out),
                   "fv_firstcal_pair_delays: null peak_bin_out, delay_bins_out, power_out, total_out or used_out");
        const bool empty = nfreqs == 0 || ntimes == 0 || nbls == 0 || npairs == 0;
        FV_REQUIRE(empty || (pair1 && pair2 && ant1 && ant2 && data), "fv_firstcal_pair_delays: null pairs or data");
        for (int i = 0; !empty && i < npairs; ++i)
            FV_REQUIRE(pair1[i] >= 0 && pair1[i] < nbls && pair2[i] >= 0 && pair2[i] < nbls,
                       "fv_firstcal_pair_delays: baseline index outside [0, nbls)");
        firstcal_pair_delays_host<decltype(real)>(device, nfreqs, ntimes, nbls, tpol, npairs, pair1, pair2, ant1, ant2, data,
                                                  data_on_device, weights, weights_on_device, pad, peak_bin_out, delay_bins_out,
                                                  power_out, total_out, used_out);
    });
}

int fv_firstcal_offsets(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, int ngroups, const int *group, const double *slopes, const void *data, int data_on_device,
                        const void *weights, int weights_on_device, void *offsets, void *uvis_out, int max_iter, double tol,
                        int *niter_out, double *change_out, double *chi2_ft_out, int *solved_out, int *vis_solved_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_firstcal_offsets: tpol must be 1 or 4");
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && (int64_t)nfreqs * ntimes < ((int64_t)1 << 31) && nbls >= 0 && nbls < ((int64_t)1 << 29),
                   "fv_firstcal_offsets: negative shape");
        FV_REQUIRE(nant >= 1, "fv_firstcal_offsets: nant must be positive");
        FV_REQUIRE(ngroups >= 1, "fv_firstcal_offsets: ngroups must be positive");
        FV_REQUIRE(max_iter >= 1, "fv_firstcal_offsets: max_iter must be positive");
        FV_REQUIRE(tol >= 0.0, "fv_firstcal_offsets: tol must be non-negative");  // (a NaN fails the comparison)
        FV_REQUIRE(((data_on_device | weights_on_device) & ~1) == 0, "fv_firstcal_offsets: the on_device flags must be 0 or 1");
        FV_REQUIRE(niter_out, "fv_firstcal_offsets: null niter_out");
        const bool empty = nfreqs == 0 || ntimes == 0;
        FV_REQUIRE(empty || (offsets && uvis_out && change_out && chi2_ft_out && solved_out && vis_solved_out),
                   "fv_firstcal_offsets: null offsets, uvis_out, change_out, chi2_ft_out, solved_out or vis_solved_out");
        FV_REQUIRE(empty || nbls == 0 || (data && ant1 && ant2 && group && slopes), "fv_firstcal_offsets: null pairs, group, slopes or data");
        if (!empty) require_pairs("fv_firstcal_offsets", nbls, nant, ant1, ant2);
        if (!empty) require_groups("fv_firstcal_offsets", nbls, ngroups, group);
        firstcal_offsets_host<decltype(real)>(device, nfreqs, ntimes, nbls, tpol, nant, ant1, ant2, ngroups, group, slopes, data,
                                              data_on_device, weights, weights_on_device, offsets, uvis_out, max_iter, tol, niter_out,
                                              change_out, chi2_ft_out, solved_out, vis_solved_out);
    });
}

int fv_abscal_slopes(int device, int precision, int nfreqs, int ntimes, int tpol, int ngroups, int per_time, const void *uvis,
                     int uvis_on_device, const void *model, int model_on_device, const void *gweights, int gweights_on_device,
                     const double *coords, int ndim, int n1, int n2, double h1, double h2, int refine, int *peak_out,
                     double *slopes_out, double *amp_out, double *power_out, double *unorm_out, double *mnorm_out, int *used_out,
                     double *chi2_ft_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_abscal_slopes: tpol must be 1 or 4");
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && (int64_t)nfreqs * ntimes < ((int64_t)1 << 29) && ngroups >= 0 && ngroups < (1 << 29),
                   "fv_abscal_slopes: negative shape");
        FV_REQUIRE(per_time == 0 || per_time == 1, "fv_abscal_slopes: per_time must be 0 or 1");
        FV_REQUIRE(ndim == 1 || ndim == 2, "fv_abscal_slopes: ndim must be 1 or 2 (a line or a planar array)");
        FV_REQUIRE(n1 >= 1 && n2 >= 1 && (n1 & 1) && (n2 & 1), "fv_abscal_slopes: n1 and n2 must be positive and odd");
        FV_REQUIRE((int64_t)n1 * n2 <= ((int64_t)1 << 22), "fv_abscal_slopes: the grid n1 n2 must not exceed 2^22 points");
        FV_REQUIRE(ndim == 2 || n2 == 1, "fv_abscal_slopes: n2 must be 1 for ndim 1");
        FV_REQUIRE(h1 > 0.0 && std::isfinite(h1) && (ndim == 1 || (h2 > 0.0 && std::isfinite(h2))),
                   "fv_abscal_slopes: the grid steps must be positive and finite");
        FV_REQUIRE(refine >= 0 && refine <= 32, "fv_abscal_slopes: refine must lie in 0 .. 32");
        FV_REQUIRE(((uvis_on_device | model_on_device | gweights_on_device) & ~1) == 0, "fv_abscal_slopes: the on_device flags must be 0 or 1");
        const bool none = nfreqs == 0 || ntimes == 0;
        FV_REQUIRE(none || (peak_out && slopes_out && amp_out && power_out && unorm_out && mnorm_out && used_out && chi2_ft_out),
                   "fv_abscal_slopes: null peak_out, slopes_out, amp_out, power_out, unorm_out, mnorm_out, used_out or chi2_ft_out");
        FV_REQUIRE(none || ngroups == 0 || (uvis && model && coords), "fv_abscal_slopes: null uvis, model or coords");
        for (int64_t i = 0; !none && i < (int64_t)ngroups * ndim; ++i)
            FV_REQUIRE(std::isfinite(coords[i]), "fv_abscal_slopes: coords must be finite");
        if (none) return;
        abscal_slopes_host<decltype(real)>(device, nfreqs, ntimes, tpol, ngroups, per_time, uvis, uvis_on_device, model, model_on_device,
                                           gweights, gweights_on_device, coords, ndim, n1, n2, h1, h2, refine, peak_out, slopes_out,
                                           amp_out, power_out, unorm_out, mnorm_out, used_out, chi2_ft_out);
    });
}

int fv_abscal_evaluate(int device, int nrows, int ngroups, const void *c, const double *coords, int ndim, const double *slopes,
                       double *out) {
    return guarded([&] {  // (everything is checked before anything runs)
        FV_REQUIRE(nrows >= 0 && nrows < (1 << 29) && ngroups >= 0 && ngroups < (1 << 29), "fv_abscal_evaluate: negative shape");
        FV_REQUIRE(ndim == 1 || ndim == 2, "fv_abscal_evaluate: ndim must be 1 or 2 (a line or a planar array)");
        FV_REQUIRE(nrows == 0 || (slopes && out), "fv_abscal_evaluate: null slopes or out");
        FV_REQUIRE(nrows == 0 || ngroups == 0 || (c && coords), "fv_abscal_evaluate: null c or coords");
        for (int64_t i = 0; nrows > 0 && i < (int64_t)ngroups * ndim; ++i)
            FV_REQUIRE(std::isfinite(coords[i]), "fv_abscal_evaluate: coords must be finite");
        abscal_evaluate_host(device, nrows, ngroups, c, coords, ndim, slopes, out);
    });
}

int fv_jones_normal_rows(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                         const void *jones, const void *vis, const void *data, const void *weights, double *A_out, void *b_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_jones_normal_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_jones_normal_rows: nant must be positive");
        FV_REQUIRE(nrows == 0 || (jones && A_out && b_out), "fv_jones_normal_rows: null jones, A_out or b_out");
        FV_REQUIRE(nrows == 0 || nbls == 0 || (vis && data && ant1 && ant2), "fv_jones_normal_rows: null pairs, vis or data");
        if (nrows > 0) require_pairs("fv_jones_normal_rows", nbls, nant, ant1, ant2);
        jones_normal_rows_host<decltype(real)>(device, nrows, nbls, nant, ant1, ant2, jones, vis, data, weights, A_out, b_out);
    });
}

int fv_jones_solve(int device, int precision, int nfreqs, int ntimes, int64_t nbls, int nant, const int *ant1, const int *ant2,
                   int per_time, const void *vis, int vis_on_device, const void *data, int data_on_device, const void *weights,
                   int weights_on_device, void *jones, int max_iter, double tol, int *niter_out, double *change_out,
                   double *chi2_ft_out, int *solved_out) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(nfreqs >= 0 && ntimes >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_jones_solve: negative shape");
        FV_REQUIRE(nant >= 1, "fv_jones_solve: nant must be positive");
        FV_REQUIRE(max_iter >= 1, "fv_jones_solve: max_iter must be positive");
        FV_REQUIRE(tol >= 0.0, "fv_jones_solve: tol must be non-negative");  // (a NaN fails the comparison)
        FV_REQUIRE(((per_time | vis_on_device | data_on_device | weights_on_device) & ~1) == 0,
                   "fv_jones_solve: per_time and the on_device flags must be 0 or 1");
        FV_REQUIRE(niter_out, "fv_jones_solve: null niter_out");
        const bool empty = nfreqs == 0 || ntimes == 0;
        FV_REQUIRE(empty || (jones && change_out && chi2_ft_out && solved_out),
                   "fv_jones_solve: null jones, change_out, chi2_ft_out or solved_out");
        FV_REQUIRE(empty || nbls == 0 || (vis && data && ant1 && ant2), "fv_jones_solve: null pairs, vis or data");
        if (!empty) require_pairs("fv_jones_solve", nbls, nant, ant1, ant2);
        jones_solve_host<decltype(real)>(device, nfreqs, ntimes, nbls, nant, ant1, ant2, per_time, vis, vis_on_device, data,
                                         data_on_device, weights, weights_on_device, jones, max_iter, tol, niter_out, change_out,
                                         chi2_ft_out, solved_out);
    });
}

int fv_weight_rows(int device, int precision, int64_t nrows, int64_t row_len, int nparts, const void *const *parts,
                   const void *weights, double *q_rows) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(nrows >= 0 && row_len >= 0, "fv_weight_rows: negative shape");
        FV_REQUIRE(nparts >= 1 && nparts <= 4 && parts, "fv_weight_rows: nparts must be 1 .. 4");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts[j], "fv_weight_rows: null part");
        FV_REQUIRE(nrows == 0 || q_rows, "fv_weight_rows: null q_rows");
        FV_HIP(hipSetDevice(device));  // (asked of an empty call too)
        weight_rows_host<decltype(real)>(device, nrows, row_len, nparts, parts, nullptr, weights, q_rows);
    });
}

int fv_gain_weight_rows(int device, int precision, int64_t nrows, int64_t nbls, int tpol, int nant, const int *ant1,
                        const int *ant2, const void *gains, const void *d_gains, int nparts, const void *const *parts, void *vis,
                        const void *weights, double *q_rows, void *hgains) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(tpol == 1 || tpol == 4, "fv_gain_weight_rows: tpol must be 1 or 4");
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_gain_weight_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_gain_weight_rows: nant must be positive");
        FV_REQUIRE(gains || nrows == 0, "fv_gain_weight_rows: null gains");
        FV_REQUIRE(nparts >= 0 && nparts <= 4 && (parts || nparts == 0), "fv_gain_weight_rows: nparts must be 0 .. 4");
        FV_REQUIRE(nparts > 0 || d_gains, "fv_gain_weight_rows: nparts == 0 needs d_gains");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts[j], "fv_gain_weight_rows: null part");
        FV_REQUIRE(vis || !(d_gains || hgains), "fv_gain_weight_rows: d_gains and hgains need vis");
        FV_REQUIRE((nrows == 0 || nbls == 0 || (ant1 && ant2)) && (nrows == 0 || q_rows), "fv_gain_weight_rows: null pairs or q_rows");
        if (nrows > 0) require_pairs("fv_gain_weight_rows", nbls, nant, ant1, ant2);
        weight_rows_host<decltype(real)>(device, nrows, tpol * nbls, nparts, parts, vis, weights, q_rows,
                                         {Cal::Gains, tpol, nant, nbls, ant1, ant2, gains, d_gains, hgains});
    });
}

int fv_jones_weight_rows(int device, int precision, int64_t nrows, int64_t nbls, int nant, const int *ant1, const int *ant2,
                         const void *jones, const void *d_jones, int nparts, const void *const *parts, void *vis,
                         const void *weights, double *q_rows, void *hjones) {
    return guarded(precision, [&](auto real) {  // (everything is checked before anything runs)
        FV_REQUIRE(nrows >= 0 && nbls >= 0 && nbls < ((int64_t)1 << 29), "fv_jones_weight_rows: negative shape");
        FV_REQUIRE(nant >= 1, "fv_jones_weight_rows: nant must be positive");
        FV_REQUIRE(jones || nrows == 0, "fv_jones_weight_rows: null jones");
        FV_REQUIRE(nparts >= 0 && nparts <= 4 && (parts || nparts == 0), "fv_jones_weight_rows: nparts must be 0 .. 4");
        FV_REQUIRE(nparts > 0 || d_jones, "fv_jones_weight_rows: nparts == 0 needs d_jones");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts[j], "fv_jones_weight_rows: null part");
        FV_REQUIRE(vis || !(d_jones || hjones), "fv_jones_weight_rows: d_jones and hjones need vis");
        FV_REQUIRE((nrows == 0 || nbls == 0 || (ant1 && ant2)) && (nrows == 0 || q_rows), "fv_jones_weight_rows: null pairs or q_rows");
        if (nrows > 0) require_pairs("fv_jones_weight_rows", nbls, nant, ant1, ant2);
        weight_rows_host<decltype(real)>(device, nrows, 4 * nbls, nparts, parts, vis, weights, q_rows,
                                         {Cal::Jones, 4, nant, nbls, ant1, ant2, jones, d_jones, hjones});
    });
}

int fv_inplace_rot(int device, int precision, const double *rot, void *b, int64_t n) {
    return guarded(precision, [&](auto real) { inplace_rot_host<decltype(real)>(device, rot, b, n); });
}

int fv_astrom_topo(int device, int precision, const double *astrom, int64_t n, const void *eq, void *topo) {
    return guarded(precision, [&](auto real) { astrom_topo_host<decltype(real)>(device, astrom, n, eq, topo); });
}

int fv_sim_create(fv_sim **h, int device, int precision, double eps, double upsampfac,
                  int polarized) {
    return guarded([&] {
        FV_REQUIRE(h, "null handle pointer");
        *h = nullptr;
        with_precision(precision, [&](auto real) {
            FV_REQUIRE(upsampfac == 2.0 || upsampfac == 1.25 || upsampfac == 0.0, "upsample factor must be 2, 1.25 or 0 (auto)");
            FV_REQUIRE(eps > 0 && eps < 1, "eps must be in (0, 1)");
            std::unique_ptr<fv_sim> s(new fv_sim());
            s->precision = precision;
            s->impl.reset(new Sim<decltype(real)>(device, eps, upsampfac, polarized));
            *h = s.release();
        });
    });
}

int fv_sim_destroy(fv_sim *h) {
    return guarded([&] { delete h; });
}

#define FV_SIM_CALL(body)                      \
    return guarded([&] {                       \
        FV_REQUIRE(h && h->impl, "null handle"); \
        body;                                  \
    })

int fv_sim_set_sources(fv_sim *h, int64_t nsrc, int nfreq, const void *eq, const void *flux,
                       int polarized_sky, int on_device) {
    FV_SIM_CALL(h->impl->set_sources(nsrc, nfreq, eq, flux, polarized_sky, on_device));
}
int fv_sim_set_times(fv_sim *h, int ntimes, const double *rot) {
    FV_SIM_CALL(FV_REQUIRE(ntimes >= 0 && (rot || !ntimes), "bad times"); h->impl->set_times(ntimes, rot));
}
int fv_sim_set_astrom(fv_sim *h, int ntimes, const double *astrom) {
    FV_SIM_CALL(FV_REQUIRE(ntimes >= 1 && astrom, "bad astrometry contexts"); h->impl->set_astrom(ntimes, astrom));
}
int fv_sim_set_topo(fv_sim *h, int ntimes, int64_t nsrc, const void *topo, int on_device) {
    FV_SIM_CALL(FV_REQUIRE(ntimes >= 1 && topo, "bad topo"); h->impl->set_topo(ntimes, nsrc, topo, on_device));
}
int fv_sim_set_freqs(fv_sim *h, int nfreq, const double *freqs) {
    FV_SIM_CALL(FV_REQUIRE(nfreq >= 1 && freqs, "bad freqs"); h->impl->set_freqs(nfreq, freqs));
}
int fv_sim_set_array(fv_sim *h, const double *R, int64_t nbls, const double *bls, int is_coplanar) {
    FV_SIM_CALL(FV_REQUIRE(R && nbls >= 1 && bls, "bad array"); h->impl->set_array(R, nbls, bls, is_coplanar));
}
int fv_sim_set_array_type1(fv_sim *h, const double *basis_matrix, int64_t nbls, const int *bls_int,
                           int n_modes) {
    FV_SIM_CALL(FV_REQUIRE(basis_matrix && nbls >= 1 && bls_int, "bad lattice array"); h->impl->set_array_type1(basis_matrix, nbls, bls_int, n_modes));
}
int fv_sim_set_nbeams(fv_sim *h, int nbeams) {
    FV_SIM_CALL(FV_REQUIRE(nbeams >= 1, "need at least one beam"); h->impl->set_nbeams(nbeams));
}
int fv_sim_set_beam_airy(fv_sim *h, int beam, double diameter) {
    FV_SIM_CALL(FV_REQUIRE(diameter > 0, "diameter must be positive"); h->impl->set_beam_airy(beam, diameter, nullptr, 1.0));
}
int fv_sim_set_reference_compat(fv_sim *h, int on) { FV_SIM_CALL(h->impl->set_reference_compat(on)); }
int fv_sim_set_beam_airy_scaled(fv_sim *h, int beam, double diameter, const double *jones_scale, double power_scale) {
    FV_SIM_CALL(FV_REQUIRE(diameter > 0, "diameter must be positive");
                FV_REQUIRE(power_scale == power_scale, "NaN power factor");
                h->impl->set_beam_airy(beam, diameter, jones_scale, power_scale));
}
int fv_sim_set_beam_table(fv_sim *h, int beam, int nfreq_tab, int nza, int naz, double za_max,
                          const void *table, int order) {
    FV_SIM_CALL(FV_REQUIRE(table, "null table"); h->impl->set_beam_table(beam, nfreq_tab, nza, naz, za_max, table, order));
}
int fv_sim_set_beam_pairs(fv_sim *h, int npairs, const int *bi, const int *bj, const int64_t *off,
                          const int *idx, const signed char *flipped) {
    FV_SIM_CALL(FV_REQUIRE(npairs >= 1 && bi && bj && off, "bad pairs"); h->impl->set_beam_pairs(npairs, bi, bj, off, idx, flipped));
}
int fv_sim_set_basis(fv_sim *h, int nant, int nbasis, int nfreq, const void *coefs, const int *ant1,
                     const int *ant2) {
    FV_SIM_CALL(FV_REQUIRE(nant >= 1 && nbasis >= 1 && coefs && ant1 && ant2, "bad basis"); h->impl->set_basis(nant, nbasis, nfreq, coefs, ant1, ant2));
}
int fv_sim_set_chunking(fv_sim *h, int nchunks, double source_buffer) {
    FV_SIM_CALL(h->impl->set_chunking(nchunks, source_buffer));
}
int fv_sim_run(fv_sim *h, int t0, int t1, int f0, int f1, void *out, int out_on_device) {
    FV_SIM_CALL(FV_REQUIRE(out, "null output"); h->impl->run(t0, t1, f0, f1, out, out_on_device));
}
int fv_sim_run_into(fv_sim *h, int t0, int t1, int f0, int f1, void *out, int64_t out_f_stride, int shared) {
    return guarded([&] {
        FV_REQUIRE(h && h->impl, "null handle");
        FV_REQUIRE(out, "null output");
        FV_REQUIRE(out_f_stride >= 0, "negative channel stride");
        h->impl->out_f_stride = out_f_stride;
        h->impl->out_shared = shared;
        try {
            h->impl->run(t0, t1, f0, f1, out, 0);
        } catch (...) {  // the layout belongs to this call only
            h->impl->out_f_stride = 0;
            h->impl->out_shared = 0;
            throw;
        }
    });
}
int fv_sim_run_residual(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device, const void *weights,
                        int weights_on_device, void *gvis, int gvis_on_device, double *chi2_ft) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(data && gvis && chi2_ft, "null data, gvis or chi2_ft");
        require_on_device_flags({data_on_device, weights_on_device, gvis_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.data = {data, data_on_device}, a.weights = {weights, weights_on_device}, a.gvis = {gvis, gvis_on_device};
        h->impl->residual_pass(Cal::None, t0, t1, f0, f1, a, chi2_ft);
    });
}
int fv_sim_set_gain_pairs(fv_sim *h, int nant, const int *ant1, const int *ant2) {
    FV_SIM_CALL(FV_REQUIRE(nant >= 1 && ant1 && ant2, "bad gain pairs"); h->impl->set_gain_pairs(nant, ant1, ant2));
}
int fv_sim_run_residual_gains(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device, const void *weights,
                              int weights_on_device, const void *gains, int gains_on_device, void *gvis, int gvis_on_device,
                              double *chi2_ft, void *ggains, int ggains_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(data && gains && gvis && chi2_ft, "null data, gains, gvis or chi2_ft");
        require_on_device_flags({data_on_device, weights_on_device, gains_on_device, gvis_on_device, ggains_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.data = {data, data_on_device}, a.weights = {weights, weights_on_device}, a.x = {gains, gains_on_device};
        a.gvis = {gvis, gvis_on_device}, a.grad = {ggains, ggains_on_device};
        h->impl->residual_pass(Cal::Gains, t0, t1, f0, f1, a, chi2_ft);
    });
}
int fv_sim_run_residual_jones(fv_sim *h, int t0, int t1, int f0, int f1, const void *data, int data_on_device, const void *weights,
                              int weights_on_device, const void *jones, int jones_on_device, void *gvis, int gvis_on_device,
                              double *chi2_ft, void *gjones, int gjones_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(data && jones && gvis && chi2_ft, "null data, jones, gvis or chi2_ft");
        require_on_device_flags({data_on_device, weights_on_device, jones_on_device, gvis_on_device, gjones_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.data = {data, data_on_device}, a.weights = {weights, weights_on_device}, a.x = {jones, jones_on_device};
        a.gvis = {gvis, gvis_on_device}, a.grad = {gjones, gjones_on_device};
        h->impl->residual_pass(Cal::Jones, t0, t1, f0, f1, a, chi2_ft);
    });
}
int fv_sim_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, const void *weights,
                        int weights_on_device, double *q_ft) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(nparts >= 1 && nparts <= 4 && parts_dev, "nparts must be 1 .. 4");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts_dev[j], "null part");
        FV_REQUIRE(q_ft, "null q_ft");
        require_on_device_flags({weights_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.weights = {weights, weights_on_device};
        h->impl->weight_pass(Cal::None, t0, t1, f0, f1, nparts, parts_dev, nullptr, a, q_ft);
    });
}
int fv_sim_gain_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                             const void *weights, int weights_on_device, const void *gains, int gains_on_device,
                             const void *d_gains, int d_gains_on_device, double *q_ft, void *hgains, int hgains_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(nparts >= 0 && nparts <= 4 && (parts_dev || nparts == 0), "nparts must be 0 .. 4");
        FV_REQUIRE(nparts > 0 || d_gains, "nparts == 0 needs d_gains");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts_dev[j], "null part");
        FV_REQUIRE(gains && q_ft, "null gains or q_ft");
        FV_REQUIRE(vis_dev || !(d_gains || hgains), "d_gains and hgains need vis");
        require_on_device_flags({weights_on_device, gains_on_device, d_gains_on_device, hgains_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.weights = {weights, weights_on_device}, a.x = {gains, gains_on_device}, a.dx = {d_gains, d_gains_on_device};
        a.grad = {hgains, hgains_on_device};
        h->impl->weight_pass(Cal::Gains, t0, t1, f0, f1, nparts, parts_dev, vis_dev, a, q_ft);
    });
}
int fv_sim_jones_weight_block(fv_sim *h, int t0, int t1, int f0, int f1, int nparts, void *const *parts_dev, void *vis_dev,
                              const void *weights, int weights_on_device, const void *jones, int jones_on_device,
                              const void *d_jones, int d_jones_on_device, double *q_ft, void *hjones, int hjones_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(nparts >= 0 && nparts <= 4 && (parts_dev || nparts == 0), "nparts must be 0 .. 4");
        FV_REQUIRE(nparts > 0 || d_jones, "nparts == 0 needs d_jones");
        for (int j = 0; j < nparts; ++j) FV_REQUIRE(parts_dev[j], "null part");
        FV_REQUIRE(jones && q_ft, "null jones or q_ft");
        FV_REQUIRE(vis_dev || !(d_jones || hjones), "d_jones and hjones need vis");
        require_on_device_flags({weights_on_device, jones_on_device, d_jones_on_device, hjones_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        SimBase::FitArrays a;
        a.weights = {weights, weights_on_device}, a.x = {jones, jones_on_device}, a.dx = {d_jones, d_jones_on_device};
        a.grad = {hjones, hjones_on_device};
        h->impl->weight_pass(Cal::Jones, t0, t1, f0, f1, nparts, parts_dev, vis_dev, a, q_ft);
    });
}
int fv_sim_run_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                       int gflux_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gflux, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gflux_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, accumulate != 0);
    });
}
int fv_sim_set_adjoint_path(fv_sim *h, int path) {
    FV_SIM_CALL(FV_REQUIRE(path == 0 || path == 1, "adjoint path must be 0 (type 3) or 1 (type 2)"); h->impl->adjoint_path = path);
}
int fv_sim_last_adjoint_path(fv_sim *h) {
    int path = 0;
    const int status = guarded([&] {
        FV_REQUIRE(h && h->impl, "null handle");
        path = h->impl->last_adjoint_path;
    });
    return status ? status : path;
}
int fv_sim_run_basis_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                             int gflux_on_device, void *gcoefs, int gcoefs_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis, "null adjoint input");
        FV_REQUIRE(gflux || gcoefs, "neither gradient is wanted (gflux and gcoefs are both null)");
        require_on_device_flags({gvis_on_device, gflux_on_device, gcoefs_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_basis_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, gcoefs, gcoefs_on_device,
                                   accumulate != 0);
    });
}
int fv_sim_run_position_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gbls,
                                int gbls_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gbls, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gbls_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_position_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gbls, gbls_on_device, accumulate, false);
    });
}
int fv_sim_run_source_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, double *gtopo,
                              int gtopo_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gtopo, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gtopo_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_source_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gtopo, gtopo_on_device, accumulate, false);
    });
}
int fv_sim_run_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device, const double *dtopo,
                       int dtopo_on_device, void *out, int out_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(out, "null output");
        FV_REQUIRE(dbls || dtopo, "neither tangent input is given (dbls and dtopo are both null)");
        require_on_device_flags({dbls_on_device, dtopo_on_device, out_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_tangent(t0, t1, f0, f1, dbls, dbls_on_device, dtopo, dtopo_on_device, out, out_on_device, false);
    });
}
int fv_sim_run_basis_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const void *dcoefs, int dcoefs_on_device, int ndir,
                             void *out, int out_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(out, "null output");
        FV_REQUIRE(dcoefs, "null coefficient directions (dcoefs)");
        FV_REQUIRE(ndir >= 1, "ndir must be at least 1");
        require_on_device_flags({dcoefs_on_device, out_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_basis_tangent(t0, t1, f0, f1, dcoefs, dcoefs_on_device, ndir, out, out_on_device);
    });
}
int fv_sim_run_basis_position_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device,
                                      double *gbls, int gbls_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gbls, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gbls_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_position_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gbls, gbls_on_device, accumulate, true);
    });
}
int fv_sim_run_basis_position_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dbls, int dbls_on_device,
                                      void *out, int out_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(out, "null output");
        FV_REQUIRE(dbls, "null baseline directions (dbls)");
        require_on_device_flags({dbls_on_device, out_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_tangent(t0, t1, f0, f1, dbls, dbls_on_device, nullptr, 0, out, out_on_device, true);
    });
}
int fv_sim_run_basis_source_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device,
                                    double *gtopo, int gtopo_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gtopo, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gtopo_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_source_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gtopo, gtopo_on_device, accumulate, true);
    });
}
int fv_sim_run_sky_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                           int gflux_on_device, double *gtopo, int gtopo_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gflux && gtopo, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gflux_on_device, gtopo_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_sky_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, gtopo, gtopo_on_device, accumulate,
                                 false);
    });
}
int fv_sim_run_basis_sky_adjoint(fv_sim *h, int t0, int t1, int f0, int f1, const void *gvis, int gvis_on_device, void *gflux,
                                 int gflux_on_device, double *gtopo, int gtopo_on_device, int accumulate) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(gvis && gflux && gtopo, "null adjoint input or output");
        require_on_device_flags({gvis_on_device, gflux_on_device, gtopo_on_device});
        FV_REQUIRE(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_sky_adjoint(t0, t1, f0, f1, gvis, gvis_on_device, gflux, gflux_on_device, gtopo, gtopo_on_device, accumulate,
                                 true);
    });
}
int fv_sim_run_basis_source_tangent(fv_sim *h, int t0, int t1, int f0, int f1, const double *dtopo, int dtopo_on_device,
                                    void *out, int out_on_device) {
    return guarded([&] {  // (the buffers are checked before the handle is looked at)
        FV_REQUIRE(out, "null output");
        FV_REQUIRE(dtopo, "null source directions (dtopo)");
        require_on_device_flags({dtopo_on_device, out_on_device});
        FV_REQUIRE(h && h->impl, "null handle");
        h->impl->run_tangent(t0, t1, f0, f1, nullptr, 0, dtopo, dtopo_on_device, out, out_on_device, true);
    });
}
int fv_sim_sync(fv_sim *h) { FV_SIM_CALL(h->impl->sync()); }
int fv_sim_stats(fv_sim *h, double *vals, int n) { FV_SIM_CALL(h->impl->stats(vals, n)); }
int fv_sim_reset_stats(fv_sim *h) { FV_SIM_CALL(h->impl->reset_stats()); }
int fv_sim_enable_timing(fv_sim *h, int on) { FV_SIM_CALL(h->impl->enable_timing(on)); }
int fv_sim_timing(fv_sim *h, double *ms, int n) { FV_SIM_CALL(h->impl->timing(ms, n)); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Catalog exchange over RCCL for hosts without torch.distributed (SURVEY 8 b / 8 e: one broadcast of the catalog
// from rank 0 at start, optionally only the frequency columns a rank's block needs; there is no other collective on
// the path -- every rank copies its own block of visibilities out).  librccl is opened on first use: the library
// loads, and everything else in it works, on a box without RCCL.
// ---------------------------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace fv {
struct Rccl {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    static Rccl &get() {
        static Rccl *r = [] {
            Rccl *o = new Rccl();  // never destroyed (no static destructor may call into a runtime that is gone)
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                o->lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (o->lib) break;
            }
            if (!o->lib) return o;
            auto sym = [&](const char *n) { return dlsym(o->lib, n); };
            o->GetUniqueId = reinterpret_cast<decltype(o->GetUniqueId)>(sym("ncclGetUniqueId"));
            o->CommInitRank = reinterpret_cast<decltype(o->CommInitRank)>(sym("ncclCommInitRank"));
            o->CommDestroy = reinterpret_cast<decltype(o->CommDestroy)>(sym("ncclCommDestroy"));
            o->Broadcast = reinterpret_cast<decltype(o->Broadcast)>(sym("ncclBroadcast"));
            o->Send = reinterpret_cast<decltype(o->Send)>(sym("ncclSend"));
            o->Recv = reinterpret_cast<decltype(o->Recv)>(sym("ncclRecv"));
            o->GroupStart = reinterpret_cast<decltype(o->GroupStart)>(sym("ncclGroupStart"));
            o->GroupEnd = reinterpret_cast<decltype(o->GroupEnd)>(sym("ncclGroupEnd"));
            o->GetErrorString = reinterpret_cast<decltype(o->GetErrorString)>(sym("ncclGetErrorString"));
            return o;
        }();
        if (!r->lib || !r->GetUniqueId || !r->CommInitRank || !r->CommDestroy || !r->Broadcast || !r->Send || !r->Recv ||
            !r->GroupStart || !r->GroupEnd)
            throw Error(FV_ERR_INTERNAL, "librccl.so.1 could not be opened (or lacks the nccl* entry points): no RCCL on this host");
        return *r;
    }
    void check(ncclResult_t rc, const char *what) const {
        if (rc == ncclSuccess) return;
        throw Error(FV_ERR_INTERNAL, std::string(what) + ": " + (GetErrorString ? GetErrorString(rc) : "RCCL error") + " (" +
                                         std::to_string((int)rc) + ")");
    }
};

// flux (nsrc, nfreq) of elem_words 4-byte words per entry -> the columns [f0, f1) of every source, contiguous
__global__ void k_pack_columns(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int64_t nsrc, int nfreq,
                               int elem_words, int f0, int f1) {
    const int64_t row_words = (int64_t)(f1 - f0) * elem_words;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsrc * row_words) return;
    const int64_t s = i / row_words, r = i % row_words;
    dst[i] = src[(s * nfreq + f0) * elem_words + r];
}
}  // namespace fv

struct fv_comm {
    ncclComm_t comm = nullptr;
    int device = 0, rank = 0, nranks = 1;
    hipStream_t stream = nullptr;
    fv::DevBuf staging;
};

extern "C" {

int fv_comm_unique_id(void *id_bytes) {
    return fv::guarded([&] {
        FV_REQUIRE(id_bytes, "null id buffer");
        static_assert(sizeof(ncclUniqueId) == FV_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
        ncclUniqueId id;
        fv::Rccl &r = fv::Rccl::get();
        r.check(r.GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(id_bytes, &id, sizeof(id));
    });
}

int fv_comm_init(fv_comm **c, int device, int rank, int nranks, const void *id_bytes) {
    return fv::guarded([&] {
        FV_REQUIRE(c && id_bytes, "null argument");
        FV_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "rank outside [0, nranks)");
        *c = nullptr;
        fv::Rccl &r = fv::Rccl::get();
        FV_HIP(hipSetDevice(device));
        std::unique_ptr<fv_comm> o(new fv_comm());
        o->device = device;
        o->rank = rank;
        o->nranks = nranks;
        ncclUniqueId id;
        std::memcpy(&id, id_bytes, sizeof(id));
        r.check(r.CommInitRank(&o->comm, nranks, id, rank), "ncclCommInitRank");
        FV_HIP(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
        *c = o.release();
    });
}

int fv_comm_destroy(fv_comm *c) {
    return fv::guarded([&] {
        if (!c) return;
        (void)hipSetDevice(c->device);
        if (c->stream) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipStreamDestroy(c->stream);
        }
        if (c->comm) (void)fv::Rccl::get().CommDestroy(c->comm);
        delete c;
    });
}

int fv_bcast_catalog(fv_comm *c, int root, void *eq_dev, int64_t eq_bytes, void *flux_dev, int64_t flux_bytes) {
    return fv::guarded([&] {
        FV_REQUIRE(c && c->comm, "null communicator");
        FV_REQUIRE(root >= 0 && root < c->nranks, "root outside [0, nranks)");
        FV_REQUIRE(eq_bytes >= 0 && flux_bytes >= 0 && (eq_dev || !eq_bytes) && (flux_dev || !flux_bytes), "bad buffers");
        fv::Rccl &r = fv::Rccl::get();
        FV_HIP(hipSetDevice(c->device));
        if (eq_bytes) r.check(r.Broadcast(eq_dev, eq_dev, (size_t)eq_bytes, ncclChar, root, c->comm, c->stream), "ncclBroadcast (positions)");
        if (flux_bytes) r.check(r.Broadcast(flux_dev, flux_dev, (size_t)flux_bytes, ncclChar, root, c->comm, c->stream), "ncclBroadcast (flux)");
        FV_HIP(hipStreamSynchronize(c->stream));
    });
}

int fv_scatter_flux_columns(fv_comm *c, int root, int64_t nsrc, int nfreq, int elem_bytes, const void *flux_root_dev,
                            const int *ranges, void *out_dev) {
    return fv::guarded([&] {
        FV_REQUIRE(c && c->comm, "null communicator");
        FV_REQUIRE(root >= 0 && root < c->nranks, "root outside [0, nranks)");
        FV_REQUIRE(nsrc >= 0 && nfreq >= 1 && elem_bytes >= 4 && elem_bytes % 4 == 0, "bad catalog shape");
        FV_REQUIRE(ranges, "null column ranges");
        for (int q = 0; q < c->nranks; ++q)
            FV_REQUIRE(ranges[2 * q] >= 0 && ranges[2 * q] <= ranges[2 * q + 1] && ranges[2 * q + 1] <= nfreq, "column range outside [0, nfreq]");
        const int64_t mine = (int64_t)(ranges[2 * c->rank + 1] - ranges[2 * c->rank]) * nsrc * elem_bytes;
        FV_REQUIRE(out_dev || !mine, "null output");
        FV_REQUIRE(c->rank != root || flux_root_dev || !nsrc, "the root holds the catalog");
        fv::Rccl &r = fv::Rccl::get();
        FV_HIP(hipSetDevice(c->device));
        const int ew = elem_bytes / 4;
        std::vector<int64_t> off(c->nranks + 1, 0);
        if (c->rank == root) {  // pack every rank's columns (one contiguous piece each), then send them in one group
            for (int q = 0; q < c->nranks; ++q) off[q + 1] = off[q] + (int64_t)(ranges[2 * q + 1] - ranges[2 * q]) * nsrc * elem_bytes;
            c->staging.reserve(std::max<size_t>((size_t)off[c->nranks], 16));
            for (int q = 0; q < c->nranks; ++q) {
                const int64_t words = (off[q + 1] - off[q]) / 4;
                if (!words) continue;
                hipLaunchKernelGGL(fv::k_pack_columns, dim3((unsigned)fv::cdiv(words, 256)), dim3(256), 0, c->stream,
                                   static_cast<const uint32_t *>(flux_root_dev),
                                   reinterpret_cast<uint32_t *>(static_cast<char *>(c->staging.p) + off[q]), nsrc, nfreq, ew,
                                   ranges[2 * q], ranges[2 * q + 1]);
            }
            FV_HIP(hipGetLastError());
        }
        r.check(r.GroupStart(), "ncclGroupStart");
        if (c->rank == root)
            for (int q = 0; q < c->nranks; ++q)
                if (off[q + 1] > off[q])
                    r.check(r.Send(static_cast<char *>(c->staging.p) + off[q], (size_t)(off[q + 1] - off[q]), ncclChar, q, c->comm, c->stream), "ncclSend");
        if (mine) r.check(r.Recv(out_dev, (size_t)mine, ncclChar, root, c->comm, c->stream), "ncclRecv");
        r.check(r.GroupEnd(), "ncclGroupEnd");
        FV_HIP(hipStreamSynchronize(c->stream));
    });
}

}  // extern "C"

#ifdef FV_FFT_STAMPS
// diagnostic builds only (see fv_nufft.h): copies out up to max_waves records of 10 values and resets the counter
extern "C" int fv_debug_stamps(unsigned long long *out, int max_waves) {
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(fv::fv_stamp_count), sizeof(n)) != hipSuccess) return -1;
    if (n > (1u << 18)) n = 1u << 18;
    if ((int)n > max_waves) n = (unsigned)max_waves;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(fv::fv_stamps), sizeof(unsigned long long) * 10 * (size_t)n) != hipSuccess) return -1;
    const unsigned int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(fv::fv_stamp_count), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}
#endif
