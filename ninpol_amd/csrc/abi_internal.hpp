// abi_internal.hpp -- what the units behind include/ninpol_amd.h share (abi_grid / abi_plan / abi_update / abi_csr / abi_apply / abi_gradient / abi_gradop / abi_jacobian / abi_jacobian_reduced / abi_jacobian_points / abi_jacobian_dirty.hip;
// exchange.hip takes the error setter): the grid behind the handle, the text of nin_last_error(), the preconditions of the entry
// points, device memory owned by the grid or by one call, and the functions of one unit that another calls.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/ninpol_amd.h"
#include "device_grid.hpp"
#include "gls_adjoint.hpp"
#include "grid_host.hpp"
#include "launch.hpp"

struct nin_grid {
    nin::HostGrid h;
    nin::DeviceGrid d;
    std::vector<uint8_t> node_class;  // GLS size class of every node (host copy, for target subsets)
    int coords_dim = 3;
};

#pragma GCC visibility push(hidden)   // between the library's own units: none of this is a dynamic symbol
namespace nin {

// (fail(code, fmt, ...), the setter of nin_last_error()'s text, is declared in launch.hpp: the launchers word their own HIP errors)
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return nin::fail(NIN_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// ---- preconditions ---------------------------------------------------------------------------------------------------------------
// The grid is on a device, with its launch plan; NIN_ENODEVICE and "grid is not on a device" + hint otherwise.  plan = false: a grid
// built on the device that nin_grid_to_device has not adopted yet passes too -- the form four host-side entry points have always
// had (nin_weights_host, nin_csr_compact_host, nin_interpolate_csr_host, nin_apply_fields_host); what they call refuses such a grid.
constexpr const char *kHintToDevice = " (call nin_grid_to_device first)";
constexpr const char *kHintWeights = ": the weight kernels are HIP only";
constexpr const char *kHintKernels = ": the kernels are HIP only";
int on_device(const nin_grid *g, const char *hint, bool plan = true);
// a weight launch can go: Neumann flags resident, method known, GLS has its permeability and (size) no system beyond the scratch kernel
int weights_ready(const DeviceGrid &d, int method, bool size = true);

// ---- device memory ---------------------------------------------------------------------------------------------------------------
template <class T>
int dev_alloc(DeviceGrid &d, T **ptr, size_t count) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    d.allocs.push_back(p);
    *ptr = static_cast<T *>(p);
    return 0;
}

template <class T>
int dev_upload(DeviceGrid &d, const T **ptr, const std::vector<T> &src) {
    T *p = nullptr;
    int rc = dev_alloc(d, &p, src.size());
    if (rc) return rc;
    if (!src.empty()) HIP_TRY(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *ptr = p;
    return 0;
}

// a buffer of d.allocs given back before the grid goes (hipFree waits for the device); the pointer is cleared
template <class T>
void dev_release(DeviceGrid &d, T *&p) {
    if (!p) return;
    auto it = std::find(d.allocs.begin(), d.allocs.end(), (void *)p);
    if (it != d.allocs.end()) d.allocs.erase(it);
    (void)hipFree((void *)p);
    p = nullptr;
}

// a scratch buffer of the grid with room for `count` elements: kept while it is large enough
template <class T>
int grow(DeviceGrid &d, T **buf, size_t *have, size_t count) {
    if (*buf && *have >= count) return NIN_OK;
    dev_release(d, *buf);
    *have = 0;
    const int rc = dev_alloc(d, buf, count);
    if (!rc) *have = count;
    return rc;
}

// A hipMalloc'd buffer that lives as long as one call: freed when the owner goes out of scope (hipFree waits for the device).  It
// stands where the plain pointer stood -- converts to it, and & gives the pointer's address -- so an allocation reads, and HIP_TRY
// words its error, as before.
template <class T>
struct DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(DevTmp &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~DevTmp() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
    T **operator&() { return &p; }
};

// What a host-pointer entry point stages around its device sibling: dev_stage gives `buf` room for `count` doubles (at least one)
// and, with a host array, copies its `count` values up; dev_fetch copies `count` values back down (synchronous, as hipMemcpy is)
inline int dev_stage(DevTmp<double> &buf, const double *host_or_null, size_t count) {
    HIP_TRY(hipMalloc((void **)&buf, std::max<size_t>(count, 1) * sizeof(double)));
    if (host_or_null) HIP_TRY(hipMemcpy(buf, host_or_null, count * sizeof(double), hipMemcpyHostToDevice));
    return NIN_OK;
}
inline int dev_fetch(double *host, const double *dev, size_t count) {
    HIP_TRY(hipMemcpy(host, dev, count * sizeof(double), hipMemcpyDeviceToHost));
    return NIN_OK;
}

// A stream (non-blocking) or an event (no timing) of the grid, made by the first call that needs it and never earlier: the streams a
// process has open share its hardware queues
inline int lazy_stream(void *&slot) {
    if (slot) return NIN_OK;
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    slot = s;
    return NIN_OK;
}
inline int lazy_event(void *&slot) {
    if (slot) return NIN_OK;
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    slot = e;
    return NIN_OK;
}

// NIN_TIMING=1: host-side laps of one call on stderr as "[tag] name ms", the name padded to `width`; a lap first waits for the
// streams it is given, so that it times the work it names
struct Laps {
    const char *tag;
    int width;
    bool on = getenv("NIN_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what, std::initializer_list<hipStream_t> wait_for = {}) {
        if (!on) return;
        for (hipStream_t s : wait_for) (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[%s] %-*s %.3f ms\n", tag, width, what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// NIN_TIMING=1: HIP events on the launch's stream around its three phases -- compaction + read-back, descriptor kernels, weight
// kernels -- and one line on stderr; the call then waits for its kernels (tools/time_update_fields.py --local reads the lines)
struct DirtyLaps {
    bool on = getenv("NIN_TIMING") != nullptr;
    hipStream_t stream;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit DirtyLaps(hipStream_t s) : stream(s) {}
    ~DirtyLaps() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    void mark(int i) { if (on && !e[i] && hipEventCreate(&e[i]) == hipSuccess) (void)hipEventRecord(e[i], stream); }
    void report(int64_t n) {
        if (!on || !e[0] || !e[1] || !e[2] || !e[3] || hipEventSynchronize(e[3]) != hipSuccess) return;
        float ms[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], e[i], e[i + 1]);
        fprintf(stderr, "[nin_dirty] nodes %lld compact+readback %.4f descriptors %.4f weights %.4f ms\n", (long long)n, ms[0], ms[1], ms[2]);
    }
};

// ---- one unit's functions that another calls ---------------------------------------------------------------------------------------
// abi_plan.hip: the launch plan of nin_grid_to_device; the walk over its kernels (work counters zeroed by the caller); the plan's
// kernels on lists of their own nodes
int build_gls_plan(nin_grid *g);
int gls_only();
int gls_side_begin(DeviceGrid &d, int piece, int add_neumann, double *out, double *nws, hipStream_t stream);
int gls_main(DeviceGrid &d, int piece, bool cube, int only, int add_neumann, double *out, double *nws, hipStream_t stream);
int launch_lists(DeviceGrid &d, int method, const int32_t *lists, const int32_t *off, uint32_t *desc, const size_t *desc_first,
                 int add_neumann, double *out, double *nws, hipStream_t stream, DirtyLaps *laps);
// a count of descriptor words rounded up to a 16-byte boundary: where launch_lists' callers let a kernel's descriptors begin
inline size_t desc_align(size_t words) { return (words + 3) & ~(size_t)3; }
// abi_update.hip: the host's copy of the resident flag bytes (flag_staging), brought up to date
int fetch_flag_bytes(nin_grid *g);
// abi_update.hip, for abi_apply.hip's coordinate adjoint too: inpoel / etype / inpofa on the device (DeviceGrid::up_*), brought by the
// first caller (synchronous)
int ensure_update_inputs(nin_grid *g);
// abi_update.hip: the marks of the dirty set and their header block, made if they are not there; and what a dirty launch answers when
// ids were refused since the last one -- NIN_EINVAL with the count and whose ids they can have been, the counter zeroed behind `stream`
int ensure_dirty_state(DeviceGrid &d, int64_t P);
int dirty_ids_refused(nin_grid *g, int32_t count, hipStream_t stream);
// abi_apply.hip: the adjoint's and the tangent's bins and scratch slots, and the adjoint's contribution buffer, given back
void release_adjoint_state(DeviceGrid &d);
// abi_apply.hip, for abi_jacobian.hip: the cell-major index of the esup pattern and the adjoint's bins, made if they are not there
// (both synchronise `stream` when they build)
int ensure_transpose_index(DeviceGrid &d, hipStream_t stream);
int ensure_adjoint_bins(DeviceGrid &d, hipStream_t stream);
// abi_apply.hip: what every derivative entry point begins with, in this order -- the grid on its device (kHintKernels), for the
// coordinates a 3-D grid, the GLS weights ready (of any size: the adjoint kernel has a bin for every system), the device set, the
// adjoint's bins made
int derivative_ready(nin_grid *g, hipStream_t stream, bool coordinates = false);
// abi_apply.hip: fn(b, run) for every bin of the adjoint kernel (only >= 0: for that bin alone) until one returns non-zero, which is
// handed back; an empty bin is the launcher's to skip.  adjoint_only_from_env: NIN_GLS_ADJ_ONLY, read at every call of the backward, the
// coordinate and the tangent entry points (per-bin timing: tools/time_adjoint.py), or -1; a linearisation passes -1 and does not read it
AdjBinRun adjoint_bin_run(const DeviceGrid &d, int b);
int adjoint_only_from_env();
template <class Fn>
int for_each_adjoint_bin(const DeviceGrid &d, int only, Fn fn) {
    for (int b = 0; b < kAdjBins; ++b)
        if (only < 0 || b == only)
            if (int rc = fn(b, adjoint_bin_run(d, b))) return rc;
    return 0;
}
// the adjoint kernel on every bin (only >= 0: that bin alone), the ten values of every (node, cell) pair into `contrib`; reduce: into a
// [nnz_esup][n_params] buffer through launch_gls_adjoint_reduced instead, for abi_jacobian_reduced.hip
int launch_adjoint_bins(DeviceGrid &d, int add_neumann, int only, const double *grad_csr, const double *grad_nws, double *contrib,
                        hipStream_t stream, const AdjointReduce *reduce = nullptr);

// abi_gradient.hip: the doubles behind the arguments of nin_gls_corner_gradients_* for n_fields fields -- u [n_fields][E], grad and flux
// [n_fields][nnz_esup][3], node_values [n_fields][P], node_gradient [n_fields][P][3] -- as the host entry point stages them
struct CornerGradientCounts {
    size_t u, grad, node_values, node_gradient;
};
CornerGradientCounts corner_gradient_counts(int64_t n_elems, int64_t n_points, int64_t nnz_esup, int32_t n_fields);
// what the entry points of abi_gradient.hip and abi_gradop.hip answer before they look at a device, in this order: a NULL argument, a
// count below one (`count_name` in the text), a grid that is not 3-D (`what` in the text)
inline int gradient_args(const nin_grid *g, const void *in, const void *out, int32_t n, const char *count_name, const char *what) {
    if (!g || !in || !out) return fail(NIN_EINVAL, "NULL argument");
    if (n < 1) return fail(NIN_EINVAL, "%s must be >= 1", count_name);
    if (g->h.dim != 3) return fail(NIN_EINVAL, "%s for 3-D grids only (this grid is %d-D)", what, (int)g->h.dim);
    return NIN_OK;
}

// ---- what the kept Jacobians share (abi_jacobian.hip, abi_jacobian_reduced.hip, abi_jacobian_points.hip) --------------------------------------------------
// nin_gls_jacobian, nin_gls_rjacobian and nin_gls_xjacobian begin with this; each adds the buffers it owns
struct KeptJacobian {
    nin_grid *g = nullptr;
    int device = -1;                   // the grid's, as it was at creation: a destroy does not look at the grid, which may be gone
    bool linearized = false;
    int64_t stamp[3] = {-1, -1, -1};   // the grid's (field_updates, geometry_updates, flag_updates) at the linearisation
    // the cotangent of a dirty relinearisation [nnz_esup], written for the listed rows only: made by the first one that finds no refused
    // ids and kept (a buffer per call would be freed per call, and hipFree waits for the device); every *_destroy frees it
    double *seed = nullptr;
    void record_stamp(const DeviceGrid &d) {
        stamp[0] = d.field_updates;
        stamp[1] = d.geom_updates;
        stamp[2] = d.flag_updates;
        linearized = true;
    }
};
// the body of a *_stamp call
inline int copy_stamp(const KeptJacobian *J, int64_t stamp[3]) {
    if (!J || !stamp) return fail(NIN_EINVAL, "NULL argument");
    std::copy(J->stamp, J->stamp + 3, stamp);
    return NIN_OK;
}
// jacobian_seed (abi_jacobian.hip): a linearisation can go on g (derivative_ready; coordinates: of the Jacobian in the node coordinates)
// and `seed` [nnz_esup] holds its cotangent u[esup[pos]].  jacobian_apply_ready: the arguments of an apply call, the grid on its device, a linearisation to apply.
int jacobian_seed(nin_grid *g, const double *dev_u_cells, hipStream_t stream, DevTmp<double> &seed, bool coordinates = false);
inline int jacobian_apply_ready(const KeptJacobian *J, int32_t n, const void *in, const void *out, const char *linearize_name) {
    if (n < 1) return fail(NIN_EINVAL, "n must be >= 1");
    if (!J || !in || !out) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(J->g, kHintKernels)) return rc;
    if (!J->linearized) return fail(NIN_ESTATE, "the Jacobian has not been linearised (call %s first)", linearize_name);
    return NIN_OK;
}
// abi_jacobian_dirty.hip: the body of the three *_linearize_dirty calls, nin_weights_dirty_device's contract restated for
// a kept Jacobian.  The grid's marked nodes are binned by adjoint bin on the device, the counts and the refused-id counter come back in
// one copy of kAdjDirtyHdrInts ints -- the only synchronisation, of `stream` -- the cotangent is seeded for the listed rows in J->seed and
// bin(b, run, seed) runs the object's mode of the adjoint kernel on every bin that has marked nodes: `run` is the bin's own (bytes,
// scratch) with the compacted list as its nodes.  finish (may be empty) follows the bins.  While everything is dirty full() -- the object's
// own *_linearize -- runs instead.  NIN_ESTATE before the first linearisation (the text names `linearize_name`).
struct DirtyLinearize {
    const char *linearize_name;
    bool coordinates;
    std::function<int()> full;
    std::function<int(int, const AdjBinRun &, const double *)> bin;
    std::function<int()> finish;
};
int jacobian_linearize_dirty(KeptJacobian *J, const double *dev_u_cells, hipStream_t stream, int clear, int64_t *n_rows, const DirtyLinearize &how);
// One *_linearize_dirty_host: u [E] and b [P] (may be NULL) go up, launch(dev_u, dev_b) is the device sibling on the null stream, and the call waits
int jacobian_linearize_dirty_host(KeptJacobian *J, const double *u_cells, const double *neumann_values,
                                  const std::function<int(const double *, const double *)> &launch);
// One *_apply_host or *_apply_transpose_host: `in` [n][in_per] goes up, launch(dev_in, dev_out, dev_extra) is the device sibling, `out`
// [n][out_per] comes down.  The full Jacobian's optional diff_mag is the extra pair [n][extra_per]: an input with extra_in, an output
// with extra_out; with neither the launch gets a null dev_extra
template <class Launch>
int jacobian_apply_host(const KeptJacobian *J, int32_t n, const char *linearize_name, const double *in, size_t in_per, double *out,
                        size_t out_per, const double *extra_in, double *extra_out, size_t extra_per, Launch launch) {
    if (int rc = jacobian_apply_ready(J, n, in, out, linearize_name)) return rc;
    HIP_TRY(hipSetDevice(J->g->d.device));
    const size_t k = (size_t)n;
    const bool extra = extra_in || extra_out;
    DevTmp<double> din, dout, dextra;
    if (int rc = dev_stage(din, in, in_per * k)) return rc;
    if (int rc = dev_stage(dout, nullptr, out_per * k)) return rc;
    if (extra)
        if (int rc = dev_stage(dextra, extra_in, extra_per * k)) return rc;
    if (int rc = launch(din.p, dout.p, extra ? dextra.p : nullptr)) return rc;
    if (int rc = dev_fetch(out, dout, out_per * k)) return rc;
    return extra_out ? dev_fetch(extra_out, dextra, extra_per * k) : NIN_OK;
}

// abi_gradop.hip: the sizes behind a nin_gls_gradop, in 64-bit arithmetic.  A node with ne cells owns 3 ne^2 doubles of the
// operator; n_values is their sum over the nodes (gop_ptr[P], scanned on the device).  The object holds gop [n_values], gop_ptr [P + 1]
// (int64) and pos_node [nnz_esup] (int32); dots [min(n, kGradopChunk)][nnz_esup] is the transposed product's scratch
inline int64_t gradop_block_values(int64_t ne) { return 3 * ne * ne; }
struct GradopBytes {
    int64_t gop, gop_ptr, pos_node;
};
inline GradopBytes gradop_bytes(int64_t n_values, int64_t n_points, int64_t nnz_esup) {
    return {8 * n_values, 8 * (n_points + 1), 4 * nnz_esup};
}
inline size_t gradop_dots_count(int64_t nnz_esup, int32_t n) { return (size_t)std::min<int32_t>(n, kGradopChunk) * (size_t)nnz_esup; }

}  // namespace nin
#pragma GCC visibility pop

// The corner-gradient operator a caller keeps (abi_gradop.hip; here so that tools/sanitize_gradop_driver.hip can stand one on a host-only
// grid).  `linearized` and `stamp` of KeptJacobian are those of the last factorisation
struct nin_gls_gradop : nin::KeptJacobian {
    int64_t *gop_ptr = nullptr;    // [P + 1], made at creation from the connectivity alone
    int32_t *pos_node = nullptr;   // [nnz_esup]
    double *gop = nullptr;         // [n_values]
    double *dots = nullptr;        // the transposed product's scratch, made by the first call and grown to the largest chunk seen
    int32_t dots_n = 0;
    int64_t n_values = 0, nnz = 0, points = 0, elems = 0;   // (of the grid at creation)
};
