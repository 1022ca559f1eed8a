// Host-side sanitizer check of libfftvis_hip's C ABI (ASan / UBSan on the CPU build).
// Built and run by `make -C oracle sanitize` against a copy of the library whose HOST code is compiled with
// -fsanitize=address,undefined (device code is not instrumented: GPU sanitizers are unavailable on this pool).
// Exercises every entry point's argument checking and error reporting -- the paths that run before any HIP
// call -- so it needs no GPU; a box with one also passes (calls that reach the runtime then succeed or
// report FV_ERR_HIP, both accepted where noted).
#include "../include/fftvis_hip.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);  \
            ++fails;                                                     \
        }                                                                \
    } while (0)

int main() {
    EXPECT(fv_version() >= 100);
    int ndev = -1;
    EXPECT(fv_device_count(&ndev) == FV_OK && ndev >= 0);
    EXPECT(fv_device_count(nullptr) == FV_ERR_ARG);
    EXPECT(std::strlen(fv_last_error()) > 0);
    int64_t b = -1;
    EXPECT(fv_device_bytes(&b) == 0 && b >= 0);
    EXPECT(fv_device_bytes(nullptr) != 0);
    EXPECT(fv_device_mem_info(0, nullptr, nullptr) == FV_ERR_ARG);

    fv_sim *h = nullptr;
    EXPECT(fv_sim_create(nullptr, 0, 2, 1e-6, 2.0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_create(&h, 0, 3, 1e-6, 2.0, 0) == FV_ERR_ARG && h == nullptr);
    EXPECT(fv_sim_create(&h, 0, 2, 0.0, 2.0, 0) == FV_ERR_ARG && h == nullptr);
    EXPECT(fv_sim_create(&h, 0, 2, 1e-6, 1.7, 0) == FV_ERR_ARG && h == nullptr);
    EXPECT(std::strstr(fv_last_error(), "upsample") != nullptr);
    // every handle call refuses a null handle before touching it
    double d9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, f[2] = {1e8, 2e8}, v[16] = {0};
    int i2[2] = {0, 0};
    int64_t off[2] = {0, 1};
    signed char fl[1] = {0};
    EXPECT(fv_sim_set_sources(nullptr, 1, 1, d9, d9, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_set_times(nullptr, 1, d9) == FV_ERR_ARG);
    EXPECT(fv_sim_set_topo(nullptr, 1, 1, d9, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_set_freqs(nullptr, 2, f) == FV_ERR_ARG);
    EXPECT(fv_sim_set_array(nullptr, d9, 1, d9, 1) == FV_ERR_ARG);
    EXPECT(fv_sim_set_array_type1(nullptr, d9, 1, i2, 1) == FV_ERR_ARG);
    EXPECT(fv_sim_set_nbeams(nullptr, 1) == FV_ERR_ARG);
    EXPECT(fv_sim_set_beam_airy(nullptr, 0, 14.0) == FV_ERR_ARG);
    EXPECT(fv_sim_set_beam_table(nullptr, 0, 1, 2, 2, 3.14, d9, 1) == FV_ERR_ARG);
    EXPECT(fv_sim_set_beam_pairs(nullptr, 1, i2, i2, off, i2, fl) == FV_ERR_ARG);
    EXPECT(fv_sim_set_basis(nullptr, 1, 1, 1, d9, i2, i2) == FV_ERR_ARG);
    EXPECT(fv_sim_set_chunking(nullptr, 1, 1.0) == FV_ERR_ARG);
    EXPECT(fv_sim_set_reference_compat(nullptr, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_set_astrom(nullptr, 1, d9) == FV_ERR_ARG);
    EXPECT(fv_astrom_topo(0, 9, d9, 1, d9, v) == FV_ERR_ARG);
    EXPECT(fv_sim_set_beam_airy_scaled(nullptr, 0, 14.0, d9, 1.0) == FV_ERR_ARG);
    EXPECT(fv_sim_run(nullptr, 0, 1, 0, 1, v, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_position_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_source_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_tangent(nullptr, 0, 1, 0, 1, v, 0, v, 0, v, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_tangent(nullptr, 0, 1, 0, 1, v, 0, 1, v, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_position_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_position_tangent(nullptr, 0, 1, 0, 1, v, 0, v, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_source_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_source_tangent(nullptr, 0, 1, 0, 1, v, 0, v, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_sky_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_sky_adjoint(nullptr, 0, 1, 0, 1, v, 0, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_sync(nullptr) == FV_ERR_ARG);
    EXPECT(fv_sim_stats(nullptr, v, 12) == FV_ERR_ARG);
    EXPECT(fv_sim_reset_stats(nullptr) == FV_ERR_ARG);
    EXPECT(fv_sim_enable_timing(nullptr, 1) == FV_ERR_ARG);
    EXPECT(fv_sim_timing(nullptr, v, 6) == FV_ERR_ARG);
    EXPECT(fv_sim_destroy(nullptr) == FV_OK);  // delete nullptr
    // stand-alone ops: argument errors come before the device is touched
    std::vector<double> x(8, 0.5), c(16, 1.0), s(4, 2.0), out(64, 0.0);
    EXPECT(fv_nufft3(0, 3, 2, 8, x.data(), x.data(), nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr, 1e-6, 2.0,
                     out.data()) == FV_ERR_ARG);
    EXPECT(fv_nufft3(0, 2, 4, 8, x.data(), x.data(), nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr, 1e-6, 2.0,
                     out.data()) == FV_ERR_ARG);
    EXPECT(fv_nufft3(0, 2, 2, -1, x.data(), x.data(), nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr, 1e-6, 2.0,
                     out.data()) == FV_ERR_ARG);
    EXPECT(fv_nufft3(0, 2, 2, 8, x.data(), nullptr, nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr, 1e-6, 2.0,
                     out.data()) == FV_ERR_ARG);
    EXPECT(fv_nudft3_direct(0, 0, 2, 8, x.data(), x.data(), nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr,
                            out.data()) == FV_ERR_ARG);
    EXPECT(fv_beam_eval(0, 2, 1, 2, 14.0, 0, 0, 0, 0.0, nullptr, 1, 0, 1.5e8, 4, x.data(), x.data(), out.data()) ==
           FV_ERR_ARG);
    EXPECT(fv_beam_eval(0, 2, 1, 0, 14.0, 0, 0, 0, 0.0, nullptr, 6, 0, 1.5e8, 4, x.data(), x.data(), out.data()) ==
           FV_ERR_ARG);
    EXPECT(fv_apparent_coherency(0, 2, 7, 4, c.data(), c.data(), x.data(), out.data()) == FV_ERR_ARG);
    EXPECT(fv_apparent_coherency(0, 5, 0, 4, c.data(), c.data(), x.data(), out.data()) == FV_ERR_ARG);
    EXPECT(fv_inplace_rot(0, 2, nullptr, x.data(), 2) == FV_ERR_ARG);
    EXPECT(fv_inplace_rot(0, 9, d9, x.data(), 2) == FV_ERR_ARG);
    // catalog exchange: argument checks come before RCCL is opened
    {
        fv_comm *cm = reinterpret_cast<fv_comm *>(0x1);
        unsigned char id[FV_COMM_ID_BYTES] = {0};
        EXPECT(fv_comm_unique_id(nullptr) == FV_ERR_ARG);
        EXPECT(fv_comm_init(nullptr, 0, 0, 1, id) == FV_ERR_ARG);
        EXPECT(fv_comm_init(&cm, 0, 0, 1, nullptr) == FV_ERR_ARG);
        EXPECT(fv_comm_init(&cm, 0, 2, 2, id) == FV_ERR_ARG);
        EXPECT(fv_comm_destroy(nullptr) == FV_OK);
        EXPECT(fv_bcast_catalog(nullptr, 0, v, 8, v, 8) == FV_ERR_ARG);
        EXPECT(fv_scatter_flux_columns(nullptr, 0, 1, 1, 8, v, i2, v) == FV_ERR_ARG);
    }
    EXPECT(fv_release_workspaces() == FV_OK);
    // the adjoint refuses null buffers and bad flags before touching the handle
    EXPECT(fv_sim_run_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, nullptr, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 2, v, 0, 0) == FV_ERR_ARG);
    // so does the basis adjoint; either of its outputs may be null, not both
    EXPECT(fv_sim_run_basis_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, nullptr, 0, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 0, nullptr, 0, nullptr, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 2, v, 0, v, 0, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 0, v, 0, v, 3, 0) == FV_ERR_ARG);
    EXPECT(fv_sim_run_basis_adjoint(reinterpret_cast<fv_sim *>(0x1), 0, 1, 0, 1, v, 0, nullptr, -1, v, 0, 0) == FV_ERR_ARG);
    // and so does the position adjoint: null buffers, on_device flags and accumulate other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        double *gb = v;
        EXPECT(fv_sim_run_position_adjoint(fake, 0, 1, 0, 1, nullptr, 0, gb, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_position_adjoint(fake, 0, 1, 0, 1, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_position_adjoint(fake, 0, 1, 0, 1, v, 2, gb, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_position_adjoint(fake, 0, 1, 0, 1, v, 0, gb, -1, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_position_adjoint(fake, 0, 1, 0, 1, v, 0, gb, 0, 2) == FV_ERR_ARG);
    }
    // and the source adjoint
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        double *gt = v;
        EXPECT(fv_sim_run_source_adjoint(fake, 0, 1, 0, 1, nullptr, 0, gt, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_source_adjoint(fake, 0, 1, 0, 1, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_source_adjoint(fake, 0, 1, 0, 1, v, 2, gt, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_source_adjoint(fake, 0, 1, 0, 1, v, 0, gt, -1, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_source_adjoint(fake, 0, 1, 0, 1, v, 0, gt, 0, 2) == FV_ERR_ARG);
    }
    // and the tangent: a null output, both inputs null (either alone may be), on_device flags other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        EXPECT(fv_sim_run_tangent(fake, 0, 1, 0, 1, v, 0, v, 0, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_tangent(fake, 0, 1, 0, 1, nullptr, 0, nullptr, 0, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_tangent(fake, 0, 1, 0, 1, v, 2, nullptr, 0, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_tangent(fake, 0, 1, 0, 1, nullptr, 0, v, -1, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_tangent(fake, 0, 1, 0, 1, v, 0, v, 0, v, 3) == FV_ERR_ARG);
    }
    // and the position passes through basis beams: null buffers, on_device flags and accumulate other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        EXPECT(fv_sim_run_basis_position_adjoint(fake, 0, 1, 0, 1, nullptr, 0, v, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_adjoint(fake, 0, 1, 0, 1, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_adjoint(fake, 0, 1, 0, 1, v, 2, v, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_adjoint(fake, 0, 1, 0, 1, v, 0, v, -1, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_adjoint(fake, 0, 1, 0, 1, v, 0, v, 0, 2) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_tangent(fake, 0, 1, 0, 1, v, 0, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_tangent(fake, 0, 1, 0, 1, nullptr, 0, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_tangent(fake, 0, 1, 0, 1, v, 2, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_position_tangent(fake, 0, 1, 0, 1, v, 0, v, 3) == FV_ERR_ARG);
    }
    // and the source passes through basis beams
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        EXPECT(fv_sim_run_basis_source_adjoint(fake, 0, 1, 0, 1, nullptr, 0, v, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_adjoint(fake, 0, 1, 0, 1, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_adjoint(fake, 0, 1, 0, 1, v, 2, v, 0, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_adjoint(fake, 0, 1, 0, 1, v, 0, v, -1, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_adjoint(fake, 0, 1, 0, 1, v, 0, v, 0, 2) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_tangent(fake, 0, 1, 0, 1, v, 0, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_tangent(fake, 0, 1, 0, 1, nullptr, 0, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_tangent(fake, 0, 1, 0, 1, v, 2, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_source_tangent(fake, 0, 1, 0, 1, v, 0, v, 3) == FV_ERR_ARG);
    }
    // and the joint sky adjoints: any null buffer, each on_device flag and accumulate other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        for (auto fn : {fv_sim_run_sky_adjoint, fv_sim_run_basis_sky_adjoint}) {
            EXPECT(fn(fake, 0, 1, 0, 1, nullptr, 0, v, 0, v, 0, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 0, nullptr, 0, v, 0, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 0, v, 0, nullptr, 0, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 2, v, 0, v, 0, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 0, v, -1, v, 0, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 0, v, 0, v, 3, 0) == FV_ERR_ARG);
            EXPECT(fn(fake, 0, 1, 0, 1, v, 0, v, 0, v, 0, 2) == FV_ERR_ARG);
        }
    }
    // and the basis tangent: a null output, null directions, ndir < 1, on_device flags other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, v, 0, 1, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, nullptr, 0, 1, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, v, 0, 0, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, v, 0, -2, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, v, 2, 1, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_run_basis_tangent(fake, 0, 1, 0, 1, v, 0, 1, v, -1) == FV_ERR_ARG);
    }
    // and the Gauss-Newton weighting: nparts outside 1 .. 4, a null part, a null q, a negative shape, a flag other than 0 or 1
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        const void *parts[4] = {v, v, v, v}, *hole[2] = {v, nullptr};
        void *dparts[4] = {v, v, v, v}, *dhole[2] = {v, nullptr};
        EXPECT(fv_weight_rows(0, 2, 1, 4, 0, parts, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_weight_rows(0, 2, 1, 4, 5, parts, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_weight_rows(0, 2, 1, 4, 1, nullptr, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_weight_rows(0, 2, 1, 4, 2, hole, nullptr, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null part") != nullptr);
        EXPECT(fv_weight_rows(0, 2, 1, 4, 1, parts, nullptr, nullptr) == FV_ERR_ARG);
        EXPECT(fv_weight_rows(0, 2, -1, 4, 1, parts, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_weight_rows(0, 3, 1, 4, 1, parts, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(nullptr, 0, 1, 0, 1, 1, dparts, nullptr, 0, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 0, dparts, nullptr, 0, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 5, dparts, nullptr, 0, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 1, nullptr, nullptr, 0, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 2, dhole, nullptr, 0, v) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 1, dparts, nullptr, 0, nullptr) == FV_ERR_ARG);
        EXPECT(fv_sim_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, 2, v) == FV_ERR_ARG);
    }
    // and the Gauss-Newton weighting with gains: tpol, shapes, nant, null gains, nparts outside 0 .. 4 or 0 without a
    // direction, a null part, a direction or a gain product without V, null pairs or q, antenna indices, flags
    {
        fv_sim *fake = reinterpret_cast<fv_sim *>(0x1);
        const void *parts[4] = {v, v, v, v}, *hole[2] = {v, nullptr};
        void *dparts[4] = {v, v, v, v}, *dhole[2] = {v, nullptr};
        const int a[3] = {0, 1, 2}, low[3] = {0, -1, 2}, high[3] = {0, 1, 3};
        EXPECT(fv_gain_weight_rows(0, 3, 1, 3, 1, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 2, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "tpol must be 1 or 4") != nullptr);
        EXPECT(fv_gain_weight_rows(0, 2, -1, 3, 1, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, -3, 1, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 0, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, nullptr, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null gains") != nullptr);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, -1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 5, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 1, nullptr, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 0, parts, v, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "nparts == 0 needs d_gains") != nullptr);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 2, hole, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null part") != nullptr);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, v, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "d_gains and hgains need vis") != nullptr);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, nullptr, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, nullptr, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, nullptr, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 4, 3, low, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_weight_rows(0, 2, 1, 3, 4, 3, a, high, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "antenna index outside [0, nant)") != nullptr);
        EXPECT(fv_sim_gain_weight_block(nullptr, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null handle") != nullptr);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, -1, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 5, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, nullptr, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 0, nullptr, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 2, dhole, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, nullptr, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, v, 0, nullptr, 0, nullptr, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, nullptr, nullptr, 0, v, 0, v, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, nullptr, nullptr, 0, v, 0, nullptr, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 2, v, 0, v, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, -1, v, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, 0, v, 3, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_gain_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, 0, v, 0, v, v, 2) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "on_device") != nullptr);
        // ... and the same with Jones matrices (no tpol: the block is polarized)
        EXPECT(fv_jones_weight_rows(0, 3, 1, 3, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, -1, 3, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, -3, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "fv_jones_weight_rows: negative shape") != nullptr);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 0, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, nullptr, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null jones") != nullptr);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, -1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 5, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 1, nullptr, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 0, parts, v, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "nparts == 0 needs d_jones") != nullptr);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 2, hole, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null part") != nullptr);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, v, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "d_jones and hjones need vis") != nullptr);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, nullptr, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, nullptr, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, a, v, nullptr, 1, parts, nullptr, nullptr, nullptr, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, low, a, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_weight_rows(0, 2, 1, 3, 3, a, high, v, nullptr, 1, parts, nullptr, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "fv_jones_weight_rows: antenna index outside [0, nant)") != nullptr);
        // (no rows and no baselines return before any device call)
        EXPECT(fv_jones_weight_rows(0, 2, 0, 3, 3, a, a, nullptr, nullptr, 1, parts, nullptr, nullptr, nullptr, nullptr) == FV_OK);
        EXPECT(fv_sim_jones_weight_block(nullptr, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null handle") != nullptr);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, -1, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 5, dparts, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, nullptr, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 0, nullptr, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "nparts == 0 needs d_jones") != nullptr);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 2, dhole, v, nullptr, 0, v, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, nullptr, 0, nullptr, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, nullptr, 0, v, 0, nullptr, 0, nullptr, nullptr, 0) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "null jones or q_ft") != nullptr);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, nullptr, nullptr, 0, v, 0, v, 0, v, nullptr, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, nullptr, nullptr, 0, v, 0, nullptr, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "d_jones and hjones need vis") != nullptr);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 2, v, 0, v, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, -1, v, 0, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, 0, v, 3, v, v, 0) == FV_ERR_ARG);
        EXPECT(fv_sim_jones_weight_block(fake, 0, 1, 0, 1, 1, dparts, v, v, 0, v, 0, v, 0, v, v, 2) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "on_device") != nullptr);
    }
    // and the gain solve: tpol, shapes, nant, antenna indices, null pointers, flags, max_iter, tol; without a baseline
    // both return before any device call
    {
        const int a[3] = {0, 1, 2}, low[3] = {0, -1, 2}, high[3] = {0, 1, 3};
        int niter = -1, solved[6] = {7, 7, 7, 7, 7, 7};
        EXPECT(fv_gain_normal_rows(0, 3, 1, 3, 1, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 2, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "fv_gain_normal_rows: tpol must be 1 or 4") != nullptr);
        EXPECT(fv_gain_normal_rows(0, 2, -1, 3, 1, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, -3, 1, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 0, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, a, a, nullptr, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, a, a, v, v, v, nullptr, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, a, a, v, v, v, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, nullptr, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, a, a, v, nullptr, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 1, 3, a, a, v, v, nullptr, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 4, 3, low, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_gain_normal_rows(0, 2, 1, 3, 4, 3, a, high, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "antenna index outside [0, nant)") != nullptr);
        double num[12], den[6];
        EXPECT(fv_gain_normal_rows(0, 2, 2, 0, 1, 3, nullptr, nullptr, v, nullptr, nullptr, nullptr, num, den) == FV_OK);
        EXPECT(num[11] == 0.0 && den[5] == 0.0);
        EXPECT(fv_gain_solve(0, 3, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 2, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, -1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, -1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, -3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 0, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 0, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "max_iter must be positive") != nullptr);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, -1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, __builtin_nan(""), &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "tol must be non-negative") != nullptr);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 2, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 2, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, -1, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 3, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "must be 0 or 1") != nullptr);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, nullptr, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, nullptr, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, nullptr, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, nullptr, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, nullptr, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, nullptr, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 1, 3, a, a, 0, v, 0, nullptr, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 4, 3, low, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_gain_solve(0, 2, 1, 1, 3, 4, 3, a, high, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(niter == -1);
        double gains[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, change[2] = {7, 7}, chi2[2] = {7, 7};
        EXPECT(fv_gain_solve(0, 1, 1, 2, 0, 1, 3, nullptr, nullptr, 1, nullptr, 0, nullptr, 0, nullptr, 0, gains, 5, 0.0, &niter, change,
                             chi2, solved) == FV_OK);
        EXPECT(niter == 0 && gains[11] == 12 && change[1] == 0 && chi2[1] == 0 && solved[5] == 0);
    }
    // and the Jones solve: the same checks without tpol; without a baseline both return before any device call
    {
        const int a[3] = {0, 1, 2}, low[3] = {0, -1, 2}, high[3] = {0, 1, 3};
        int niter = -1, solved[12];
        EXPECT(fv_jones_normal_rows(0, 3, 1, 3, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, -1, 3, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, -3, 3, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "fv_jones_normal_rows: negative shape") != nullptr);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 0, a, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, a, nullptr, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, a, v, v, v, nullptr, nullptr, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, a, v, v, v, nullptr, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, nullptr, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, a, v, nullptr, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, a, v, v, nullptr, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, low, a, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(fv_jones_normal_rows(0, 2, 1, 3, 3, a, high, v, v, v, nullptr, v, v) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "antenna index outside [0, nant)") != nullptr);
        double A[48], b[48];
        A[47] = b[47] = 7.0;
        EXPECT(fv_jones_normal_rows(0, 2, 2, 0, 3, nullptr, nullptr, v, nullptr, nullptr, nullptr, A, b) == FV_OK);
        EXPECT(A[47] == 0.0 && b[47] == 0.0);
        EXPECT(fv_jones_solve(0, 3, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, -1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, -1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, -3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 0, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 0, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "fv_jones_solve: max_iter must be positive") != nullptr);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, -1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, __builtin_nan(""), &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "tol must be non-negative") != nullptr);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 2, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 2, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, -1, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 3, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(std::strstr(fv_last_error(), "must be 0 or 1") != nullptr);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, nullptr, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, nullptr, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, nullptr, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, nullptr, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, nullptr) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, nullptr, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, nullptr, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, a, 0, v, 0, nullptr, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, low, a, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(fv_jones_solve(0, 2, 1, 1, 3, 3, a, high, 0, v, 0, v, 0, nullptr, 0, v, 5, 1e-8, &niter, v, v, solved) == FV_ERR_ARG);
        EXPECT(niter == -1);
        double jones[48], change[2] = {7, 7}, chi2[2] = {7, 7};
        for (int i = 0; i < 48; ++i) jones[i] = i + 1;
        for (int i = 0; i < 12; ++i) solved[i] = 7;
        EXPECT(fv_jones_solve(0, 1, 1, 2, 0, 3, nullptr, nullptr, 1, nullptr, 0, nullptr, 0, nullptr, 0, jones, 5, 0.0, &niter, change,
                              chi2, solved) == FV_OK);
        EXPECT(niter == 0 && jones[47] == 48 && change[1] == 0 && chi2[1] == 0 && solved[11] == 0);
    }
    // a call that gets past the argument checks reports the missing device as a HIP error, not a crash
    if (ndev == 0) {
        EXPECT(fv_sim_create(&h, 0, 2, 1e-6, 2.0, 1) == FV_ERR_HIP && h == nullptr);
        EXPECT(fv_nufft3(0, 2, 2, 8, x.data(), x.data(), nullptr, c.data(), 1, 4, s.data(), s.data(), nullptr, 1e-6, 2.0,
                         out.data()) == FV_ERR_HIP);
    }
    std::printf(fails ? "abi_sanitize_check: %d failure(s)\n" : "abi_sanitize_check: ok\n", fails);
    return fails ? 1 : 0;
}
