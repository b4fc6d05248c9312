// abi_plan.hip -- the C ABI, part 2: the GLS launch plan (gls_plan.hpp) -- built when the grid goes to the device, walked by every
// weight launch -- with nin_weights_device / nin_weights_host and the plan's node and flop counts.
#include <hipcub/hipcub.hpp>
#include <cmath>

#include "abi_internal.hpp"
#include "hex8_desc.hpp"
#include "mfw_desc.hpp"
#include "mfg_desc.hpp"
#include "mfx_desc.hpp"
#include "quad4_desc.hpp"

using namespace nin;

namespace {

// ---- locality order of a kernel's node list --------------------------------------------------------------------------------
// A list in node order walks the mesh the way its nodes are numbered (a structured mesh: along x, row by row, plane by plane),
// and a node shares its cells and faces with neighbours that are a whole plane of the numbering away: with 2 x 256 groups of
// the cube-node kernel in flight per XCD the data comes in again for every plane (FETCH_SIZE 3.58 GiB per launch at 216^3
// against 2.6 with half as many waves).  So the list is reordered by where the nodes ARE -- inside each piece of interpolate()'s
// pipeline, whose pieces stay sub-ranges of the list:
//   default   strips of 16 mesh rows (axis 1 quantised to ~cbrt(P) levels) walked plane by plane (axis 2), node order inside:
//             the rows a plane apart meet in the 4 MB L2 and the requests stay as coalesced as the numbering makes them --
//             FETCH_SIZE 3.58 -> 1.97 GiB (traffic = the algorithmic bytes), 4.90 -> 4.78 ms in one session (s4 / s8 / s32: 4.84 /
//             4.85 / 4.82);
//   "m"       Morton order of the coordinates (10 bits an axis over the bounding cube): 3.05 GiB but 1.6 % SLOWER than node order
//             -- uncoalesced requests are instructions too, and the kernel is bound by what it issues;
//   "off"     node order.
// Any order gives the same weights bit for bit (a node's arithmetic does not depend on its neighbours in the list; tested).
// Runs of 16 consecutive entries (one pass of a 16-nodes-per-wavefront kernel) move as one: inside a run the rows of the CSR
// tables and of the output stay next to each other -- single nodes in Morton order cost more in uncoalesced requests than
// the order saves (5.09 against 4.83 ms at 216^3, measured; runs of 64 / 256 are slower still).
#ifndef NIN_LOCALITY_RUN
#define NIN_LOCALITY_RUN 16
#endif
constexpr int kLocalityRun = NIN_LOCALITY_RUN;
__device__ __forceinline__ uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// strip > 0: instead, strips of `strip` mesh rows (axis 1 at ~cbrt(P) levels) walked plane by plane (axis 2), node order inside:
// the rows a plane apart meet in the L2 while the requests stay as coalesced as the numbering makes them
__global__ void k_locality_keys(const double *__restrict__ coords, const int32_t *__restrict__ nodes, int32_t count, double lo,
                                double scale, int32_t c1, int32_t c2, int32_t c3, int32_t strip, double lscale,
                                uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t p = nodes[i & ~(int64_t)(kLocalityRun - 1)];   // the key of the run's first entry: the (stable) sort moves whole runs
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double t = (coords[3 * (size_t)p + k] - lo) * scale;
        q[k] = t > 0.0 ? (t < 1023.0 ? (uint32_t)t : 1023u) : 0u;
    }
    const int32_t self = nodes[i];
    const uint32_t piece = (uint32_t)(self >= c1) + (uint32_t)(self >= c2) + (uint32_t)(self >= c3);
    if (strip > 0) {
        const double ty = (coords[3 * (size_t)p + 1] - lo) * lscale, tz = (coords[3 * (size_t)p + 2] - lo) * lscale;
        const uint32_t yq = ty > 0.0 ? (ty < 32767.0 ? (uint32_t)(ty + 0.5) : 32767u) : 0u;
        const uint32_t zq = tz > 0.0 ? (tz < 32767.0 ? (uint32_t)(tz + 0.5) : 32767u) : 0u;
        keys[i] = (piece << 30) | ((yq / (uint32_t)strip) << 15) | zq;
        return;
    }
    keys[i] = (piece << 30) | spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
}
// `list` (device, count entries, ascending node ids) -> the same entries in locality order; pieces = the pipeline's node boundaries
int locality_order(const DeviceGrid &d, int32_t *list, int32_t count, const int32_t *chunk_node) {
    if (count < 2048) return NIN_OK;
    double lo = 0.0, hi = 0.0;
    {   // the bounding cube: smallest and largest coordinate of any axis
        DevTmp<double> mm;
        DevTmp<void> rt;
        size_t rb = 0, rb2 = 0;
        const int n3 = 3 * d.v.n_points;
        bool ok = hipMalloc((void **)&mm, 16) == hipSuccess &&
                  hipcub::DeviceReduce::Min(nullptr, rb, d.v.coords, mm.p, n3) == hipSuccess &&
                  hipcub::DeviceReduce::Max(nullptr, rb2, d.v.coords, mm.p + 1, n3) == hipSuccess &&
                  hipMalloc(&rt, rb > rb2 ? rb : rb2) == hipSuccess;
        rb = rb > rb2 ? rb : rb2;
        ok = ok && hipcub::DeviceReduce::Min(rt, rb, d.v.coords, mm.p, n3) == hipSuccess &&
             hipcub::DeviceReduce::Max(rt, rb, d.v.coords, mm.p + 1, n3) == hipSuccess;
        double h2[2] = {0.0, 0.0};
        ok = ok && hipMemcpy(h2, mm, 16, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) return fail(NIN_EHIP, "locality order: bounding cube: %s", hipGetErrorString(hipGetLastError()));
        lo = h2[0]; hi = h2[1];
    }
    if (!(hi > lo)) return NIN_OK;
    DevTmp<uint32_t> keys, keys_out;
    DevTmp<int32_t> list_out;
    DevTmp<void> tmp;
    size_t tmp_bytes = 0;
    int rc = NIN_OK;
    auto step = [&](hipError_t e) { if (e != hipSuccess && rc == NIN_OK) rc = fail(NIN_EHIP, "locality order: %s", hipGetErrorString(e)); return e == hipSuccess; };
    if (step(hipMalloc((void **)&keys, (size_t)count * 4)) && step(hipMalloc((void **)&keys_out, (size_t)count * 4)) &&
        step(hipMalloc((void **)&list_out, (size_t)count * 4))) {
        const char *mode = getenv("NIN_GLS_LOCALITY_ORDER");
        const int32_t strip = !mode ? 16 : mode[0] == 's' ? (mode[1] ? atoi(mode + 1) : 16) : 0;   // default: strips of 16 rows; "m": Morton
        const double levels = std::cbrt((double)d.v.n_points) - 1.0;                          // mesh intervals per axis of a cube of this many nodes
        hipLaunchKernelGGL(k_locality_keys, blocks_for(count), dim3(256), 0, nullptr, d.v.coords, list, count, lo,
                           1024.0 / (hi - lo), chunk_node[1], chunk_node[2], chunk_node[3], strip, (levels > 1.0 ? levels : 1.0) / (hi - lo), keys.p);
        if (step(hipGetLastError()) && step(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, keys_out.p, list, list_out.p, count)) &&
            step(hipMalloc(&tmp, tmp_bytes)) &&
            step(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys.p, keys_out.p, list, list_out.p, count)))
            (void)step(hipMemcpy(list, list_out, (size_t)count * 4, hipMemcpyDeviceToDevice));
    }
    return rc;
}

// ---- the GLS launch plan (gls_plan.hpp): the two functions that switch over the launcher family -------------------------------
static_assert(kGlsDescHex8 == kHex8DescWords && kGlsDescQuad4 == kQuad4DescWords && kGlsDescMfw == kMfwDescWords &&
                  kGlsDescMfx == kMfxDescWords && kGlsDescMfg == kMfgDescWords, "gls_plan.hpp's descriptor sizes are not the descriptor headers'");

// the descriptors of `count` entries of a list of plan kernel k's nodes: gls_plan_row(k).desc_words words an entry
int launch_plan_desc(const DeviceGrid &d, GlsKernel k, const int32_t *nodes, int32_t count, uint32_t *desc, hipStream_t stream) {
    if (count <= 0) return 0;
    switch (gls_plan_row(k).family) {
        case GlsFamily::hex8: return launch_hex8_desc(d.v, nodes, count, reinterpret_cast<int32_t *>(desc), stream);
        case GlsFamily::quad4: return launch_quad4_desc(d.v, nodes, count, reinterpret_cast<int32_t *>(desc), stream);
        case GlsFamily::mfw: return launch_mfw_desc(d.v, nodes, count, desc, stream);
        case GlsFamily::mfx: return launch_mfx_desc(d.v, nodes, count, desc, stream);
        case GlsFamily::mfg: return launch_mfg_desc(d.v, nodes, count, desc, stream);
        default: return 0;   // the kernel reads no descriptors
    }
}

// plan kernel k on `count` entries of a list of its nodes and their descriptors (nodes == nullptr: the block / scratch kernels walk
// 0 .. count - 1).  The block / scratch parameters are the plan's own list's; the work counter is the table's.
int launch_plan_kernel(const DeviceGrid &d, GlsKernel k, const int32_t *nodes, const uint32_t *desc, int32_t count, int add_neumann,
                       double *out, double *nws, hipStream_t stream) {
    const GlsPlanRow r = gls_plan_row(k);
    const DeviceGrid::GlsList &l = d.plan[k];
    int32_t *queue = r.counter >= 0 ? d.gls_queue + r.counter : nullptr;
    const int32_t *idesc = reinterpret_cast<const int32_t *>(desc);
    switch (r.family) {
        case GlsFamily::block: return launch_gls_block(d.v, nodes, count, l.waves, l.col_slots, l.lds_bytes, add_neumann, out, nws, queue, stream);
        case GlsFamily::scratch:
            return launch_gls_class(d.v, nodes, count, 0, l.rows_per_lane, add_neumann, out, nws, d.gls_scratch, d.gls_scratch_stride,
                                    d.gls_scratch_slots, stream);
        case GlsFamily::hex8: return launch_gls_hex8mf(d.v, nodes, idesc, count, add_neumann, out, nws, queue, stream);
        case GlsFamily::mfw: return launch_gls_mfw(d.v, nodes, desc, count, r.sub, add_neumann, out, nws, queue, stream);
        case GlsFamily::small: return launch_gls_small(d.v, nodes, count, r.sub, add_neumann, out, nws, stream);
        case GlsFamily::quad4: return launch_gls_quad4(d.v, nodes, idesc, count, add_neumann, out, nws, stream);
        case GlsFamily::mfx: return launch_gls_mfx(d.v, nodes, desc, count, r.sub, add_neumann, out, nws, queue, stream);
        case GlsFamily::mfg: return launch_gls_mfg(d.v, nodes, desc, count, add_neumann, out, nws, queue, d.mfg_tiles, d.mfg_slots, stream);
    }
    return fail(NIN_EINVAL, "the GLS launch plan has no kernel family %d", (int)r.family);
}

}  // namespace

// nin_grid_to_device's launch plan: the nodes binned by kernel (classified on the device), every list with its descriptors and its
// cuts for interpolate()'s pipeline
int nin::build_gls_plan(nin_grid *g) {
    DeviceGrid &d = g->d;
    const int64_t P = g->h.n_points;
    int rc;
    g->node_class.assign((size_t)P, 0);
    // debugging switches: keep nodes away from a kernel (gls_plan.hpp: GlsRoute)
    auto unless = [](const char *name, int bit) { return getenv(name) == nullptr ? bit : 0; };
    const int use_group = unless("NIN_GLS_NO_GROUP", kRouteHex8) | unless("NIN_GLS_NO_MFW", kRouteMfw) |
                          unless("NIN_GLS_NO_MFW_GENERAL", kRouteMfwGeneral) | unless("NIN_GLS_NO_SMALL", kRouteSmall) |
                          unless("NIN_GLS_NO_QUAD4", kRouteQuad4) | unless("NIN_GLS_NO_MFX", kRouteMfx) |
                          unless("NIN_GLS_NO_MFX_7X12", kRouteMfx7x12) | unless("NIN_GLS_NO_MFX_SMALL", kRouteMfxSmall) |
                          unless("NIN_GLS_NO_MFG", kRouteMfg) | (getenv("NIN_GLS_MFX_NO_BOUNDARY") != nullptr ? kRouteMfxNoBoundary : 0) |
                          unless("NIN_GLS_MFW_GENERAL", kRouteMfxTakesGeneral);
    const bool force_global = getenv("NIN_GLS_FORCE_GLOBAL") != nullptr;   // testing switch: systems in global scratch
    int64_t need_max[kGlsClasses] = {0}, rows_max[kGlsClasses] = {0}, cols_max[kGlsClasses] = {0};
    {
        uint8_t *dcls = nullptr;   // stays resident (P bytes): a dirty launch bins its nodes on the device (fields_scatter.hip)
        DevTmp<unsigned long long> dmax;
        unsigned long long hmax[3 * kGlsClasses];
        if ((rc = dev_alloc(d, &dcls, (size_t)P))) return rc;
        d.node_class = dcls;
        if (hipMalloc((void **)&dmax, sizeof hmax) != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc");
        hipError_t e1 = hipMemset(dmax, 0, sizeof hmax);
        const int lrc = launch_classify(d.v, use_group, force_global, dcls, dmax, nullptr);
        if (e1 == hipSuccess) e1 = hipMemcpy(g->node_class.data(), dcls, (size_t)P, hipMemcpyDeviceToHost);
        if (e1 == hipSuccess) e1 = hipMemcpy(hmax, dmax, sizeof hmax, hipMemcpyDeviceToHost);
        if (lrc || e1 != hipSuccess) return fail(NIN_EHIP, "node classification: %s", hipGetErrorString(e1));
        for (int c = 0; c < kGlsClasses; ++c) { need_max[c] = (int64_t)hmax[3 * c]; rows_max[c] = (int64_t)hmax[3 * c + 1]; cols_max[c] = (int64_t)hmax[3 * c + 2]; }
    }
    std::vector<int32_t> lists[kGlsPlanKernels];
    {
        int8_t kernel_of[256];
        for (int c = 0; c < 256; ++c) kernel_of[c] = (int8_t)gls_class_kernel(c);
        for (int64_t p = 0; p < P; ++p) {
            const int k = kernel_of[g->node_class[p]];
            if (k < 0) return fail(NIN_EHIP, "node classification: class byte %d belongs to no kernel", (int)g->node_class[p]);
            lists[k].push_back((int32_t)p);
        }
        // every node the cube-node kernel does not take, ascending: what the fused apply leaves to the list kernel
        std::vector<int32_t> rest;
        rest.reserve((size_t)P - lists[gk::hex8].size());
        for (int64_t p = 0; p < P; ++p)
            if (g->node_class[p] != gls_class_byte(gk::hex8)) rest.push_back((int32_t)p);
        d.noncube_count = (int32_t)rest.size();
        const int32_t *lp = nullptr;
        if (d.noncube_count && (rc = dev_upload(d, &lp, rest))) return rc;
        d.noncube_nodes = lp;
        d.noncube_nodes_ready = true;
    }
    for (int c = 0; c < kGlsClasses; ++c) {   // the block kernel's classes and the scratch class: plan kernels 0 .. kGlsClasses - 1
        auto &k = d.plan[c];
        k.lds_bytes = c == kGlsClasses - 1 ? 0 : (int32_t)need_max[c];
        k.rows_per_lane = (int32_t)std::max<int64_t>(1, (rows_max[c] + 63) / 64);
        k.waves = gls_class_waves(c);
        k.col_slots = (int32_t)std::max<int64_t>(1, (cols_max[c] + 63) / 64);
    }
    // interpolate()'s pipeline: its pieces' node boundaries (multiples of 64 nodes)
    constexpr int K = DeviceGrid::kE2eChunks;
    for (int j = 0; j <= K; ++j) d.chunk_node[j] = j == K ? (int32_t)P : (int32_t)((P * j / K) & ~(int64_t)63);
    // (NIN_GLS_LOCALITY_ORDER: "s<rows>" = strips of that many mesh rows, the default s16; "m" = Morton order; "off" = node order)
    const char *lo_env = getenv("NIN_GLS_LOCALITY_ORDER");
    const bool locality = !(lo_env && (lo_env[0] == 'o' || lo_env[0] == '0'));
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        auto &l = d.plan[k];
        l.count = (int32_t)lists[k].size();
        // where the pieces' boundaries fall in the list (ascending here on the host; a list in locality order on the device is
        // permuted inside the pieces only)
        for (int j = 0; j <= K; ++j) l.chunk_off[j] = (int32_t)(std::lower_bound(lists[k].begin(), lists[k].end(), d.chunk_node[j]) - lists[k].begin());
        if (!l.count) continue;
        const int32_t *lp = nullptr;
        if ((rc = dev_upload(d, &lp, lists[k]))) return rc;
        l.nodes = const_cast<int32_t *>(lp);
        if (k == gk::hex8 && locality && (rc = locality_order(d, l.nodes, l.count, d.chunk_node))) return rc;
        if (const int words = gls_plan_row(k).desc_words) {   // one record per list entry
            if ((rc = dev_alloc(d, &l.desc, (size_t)l.count * words))) return rc;
            if (launch_plan_desc(d, GlsKernel(k), l.nodes, l.count, l.desc, nullptr)) return fail(NIN_EHIP, "descriptor kernel of plan kernel %d", k);
        }
    }
    if (d.plan[gk::mfg_tiles].count) {   // one slot of tiles per resident wavefront
        d.mfg_slots = std::min<int32_t>(d.plan[gk::mfg_tiles].count, kMfgResidentWaves);
        if ((rc = dev_alloc(d, &d.mfg_tiles, (size_t)d.mfg_slots * kMfgSlotDoubles))) return rc;
    }
    d.gls_too_large = rows_max[gk::scratch] > 1024;
    if ((rc = dev_alloc(d, &d.gls_queue, (size_t)kGlsQueueInts))) return rc;
    if (d.plan[gk::scratch].count) {
        d.gls_scratch_slots = std::min<int32_t>(d.plan[gk::scratch].count, 512);   // one per resident team (kernels_gls.hip)
        d.gls_scratch_stride = need_max[gk::scratch] / 8;
        if ((rc = dev_alloc(d, &d.gls_scratch, (size_t)d.gls_scratch_slots * d.gls_scratch_stride))) return rc;
    }
    const char *mn = getenv("NIN_E2E_MIN_NODES");                                // (tests: the pipeline on small meshes too)
    d.chunkable = P >= (mn ? atoll(mn) : 64 * 1024) && P >= 64 * K && getenv("NIN_E2E_NO_PIPELINE") == nullptr;   // small meshes: one piece
    // a single class holding every node in order needs no list: the kernel walks 0..P-1 directly
    for (int c = 0; c < kGlsClasses; ++c)
        if (d.plan[c].count == P) { d.plan[c].nodes = nullptr; d.chunkable = false; }
    return NIN_OK;
}

// ---- one launch of the plan: every walk over its kernels goes through the two arrays below ---------------------------------------
// The long poles first, on the side stream when it is on (a node on global-memory tiles takes ~0.5 ms, one of the global-scratch class ~2 ms,
// on a wavefront of its own); then kMainOrder, where the two come up again for a launch whose side stream did not take them.
static constexpr GlsKernel kSideOrder[] = {gk::mfg_tiles, gk::scratch};
static constexpr GlsKernel kMainOrder[] = {gk::hex8,     gk::mfw_large, gk::mfw_small, gk::mfw_general, gk::small4,       gk::small8,
                                           gk::small12,  gk::quad4,     gk::mfx_6x10,  gk::mfx_7x11,    gk::mfx_8x13,     gk::mfx_9x15,
                                           gk::mfx_10x16, gk::mfx_boundary, gk::mfx_4x7, gk::mfx_7x12,  gk::mfg_tiles,    gk::block1,
                                           gk::block2,   gk::block4,    gk::block8,    gk::scratch};
static constexpr bool main_order_is_complete() {
    unsigned seen = 0;
    for (GlsKernel k : kMainOrder) seen |= 1u << k;
    return sizeof kMainOrder / sizeof kMainOrder[0] == kGlsPlanKernels && seen == (1u << kGlsPlanKernels) - 1;
}
static_assert(main_order_is_complete(), "kMainOrder must name every kernel of the plan once");
static bool on_side_stream(GlsKernel k) { return std::find(std::begin(kSideOrder), std::end(kSideOrder), k) != std::end(kSideOrder); }

// the entries of plan kernel k's list that lie in piece `piece` of interpolate()'s pipeline (piece < 0: the whole list)
struct PlanRange { const int32_t *nodes; const uint32_t *desc; int32_t count; };
static PlanRange plan_range(const DeviceGrid &d, GlsKernel k, int piece) {
    const auto &l = d.plan[k];
    const int32_t b = piece < 0 ? 0 : l.chunk_off[piece], n = (piece < 0 ? l.count : l.chunk_off[piece + 1]) - b;
    return {l.nodes ? l.nodes + b : nullptr, l.desc ? l.desc + (size_t)gls_plan_row(k).desc_words * b : nullptr, n};
}

// kSideOrder's kernels on the side stream: ordered behind everything enqueued on `stream` so far (the zeroed work counters, the
// caller's buffers) and joined by gls_side_end.  NIN_GLS_NO_SIDE_STREAM=1: off.
int nin::gls_side_begin(DeviceGrid &d, int piece, int add_neumann, double *out, double *nws, hipStream_t stream) {
    d.side_pending = false;
    bool any = false;
    for (GlsKernel k : kSideOrder) any = any || plan_range(d, k, piece).count > 0;
    if (!any || getenv("NIN_GLS_NO_SIDE_STREAM") != nullptr) return 0;
    int rc = lazy_stream(d.side_stream);
    if (!rc) rc = lazy_event(d.ev_fork);
    if (!rc) rc = lazy_event(d.ev_join);
    if (rc) return rc;
    hipStream_t side = static_cast<hipStream_t>(d.side_stream);
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(d.ev_fork), stream));
    HIP_TRY(hipStreamWaitEvent(side, static_cast<hipEvent_t>(d.ev_fork), 0));
    for (GlsKernel k : kSideOrder) {
        const PlanRange r = plan_range(d, k, piece);
        if (!rc && r.count > 0) rc = launch_plan_kernel(d, k, r.nodes, r.desc, r.count, add_neumann, out, nws, side);
    }
    if (!rc) rc = launch_status(hipEventRecord(static_cast<hipEvent_t>(d.ev_join), side));
    d.side_pending = rc == 0;
    return rc;
}
static int gls_side_end(DeviceGrid &d, hipStream_t stream) {
    if (!d.side_pending) return 0;
    d.side_pending = false;
    HIP_TRY(hipStreamWaitEvent(stream, static_cast<hipEvent_t>(d.ev_join), 0));
    return NIN_OK;
}

// NIN_GLS_ONLY=<k>: launch only kernel k of the plan (a GlsKernel: numbered as nin_gls_plan counts them; measurement: bench.py times
// the kernels of a plan one by one; read at every launch)
int nin::gls_only() {
    const char *e = getenv("NIN_GLS_ONLY");
    return e && *e ? atoi(e) : -1;
}

// The plan's kernels on the main stream for one piece of the pipeline (piece < 0: all nodes), then the join with the side stream.  The
// work counters are zeroed by the caller; what gls_side_begin took is left out.  cube = false: without the cube-node kernel (the fused
// apply launches its own form of it); only >= 0: that kernel alone.
int nin::gls_main(DeviceGrid &d, int piece, bool cube, int only, int add_neumann, double *out, double *nws, hipStream_t stream) {
    int rc = 0;
    for (GlsKernel k : kMainOrder) {
        if ((k == gk::hex8 && !cube) || (only >= 0 && only != k) || (d.side_pending && on_side_stream(k))) continue;
        const PlanRange r = plan_range(d, k, piece);
        if (!rc && r.count > 0) rc = launch_plan_kernel(d, k, r.nodes, r.desc, r.count, add_neumann, out, nws, stream);
    }
    if (!rc) rc = gls_side_end(d, stream);
    return rc;
}

// The plan's kernels on lists of their own nodes, not the plan's: kernel k takes lists[off[k] .. off[k + 1]) and writes its
// descriptors to desc + desc_first[k] first (one descriptor launch per non-empty list, not per family: a few tiny launches more;
// desc and every desc_first[k] on a 16-byte boundary, desc_align(): the cube-node kernel fetches its records 16 bytes at a time);
// IDW / LS take all off[kGlsPlanKernels] entries as one list.  No side stream: every listed row is written by exactly one kernel,
// in any order.  laps: the dirty launch's marks (null: none).
int nin::launch_lists(DeviceGrid &d, int method, const int32_t *lists, const int32_t *off, uint32_t *desc, const size_t *desc_first,
                      int add_neumann, double *out, double *nws, hipStream_t stream, DirtyLaps *laps) {
    const bool gls = method == NIN_METHOD_GLS;
    if (laps) laps->mark(1);
    if (gls) {
        for (int k = 0; k < kGlsPlanKernels; ++k)
            if (launch_plan_desc(d, GlsKernel(k), lists + off[k], off[k + 1] - off[k], desc + desc_first[k], stream))
                return fail(NIN_EHIP, "descriptor kernel of plan kernel %d", k);
        HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
    }
    if (laps) laps->mark(2);
    int rc = 0;
    if (!gls)
        rc = method == NIN_METHOD_IDW ? launch_idw(d.v, lists, off[kGlsPlanKernels], 0, 0, out, nws, stream)
                                      : launch_ls(d.v, lists, off[kGlsPlanKernels], 0, 0, out, nws, stream);
    else
        for (GlsKernel k : kMainOrder)
            if (!rc && off[k + 1] > off[k])
                rc = launch_plan_kernel(d, k, lists + off[k], desc + desc_first[k], off[k + 1] - off[k], add_neumann, out, nws, stream);
    if (rc) return rc;
    if (laps) laps->mark(3);
    return NIN_OK;
}

int nin_weights_device(nin_grid *g, int method, const int64_t *targets, int64_t n_targets, int add_neumann,
                       double *dev_csr_data, double *dev_neumann_ws, void *stream_) {
    if (!g || !dev_csr_data || !dev_neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    int rc = on_device(g, kHintWeights);
    if (!rc) rc = weights_ready(d, method);
    if (rc) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(d.device));
    const int64_t P = g->h.n_points;
    const bool all = targets == nullptr;
    if (!all && n_targets < 0) return fail(NIN_EINVAL, "negative n_targets");
    if (all) {
        if (method == NIN_METHOD_IDW) rc = launch_idw(d.v, nullptr, (int32_t)P, (int32_t)g->h.mx_elems_per_point, d.nnz_e, dev_csr_data, dev_neumann_ws, stream);
        else if (method == NIN_METHOD_LS) rc = launch_ls(d.v, nullptr, (int32_t)P, (int32_t)g->h.mx_elems_per_point, d.nnz_e, dev_csr_data, dev_neumann_ws, stream);
        else {
            HIP_TRY(hipMemsetAsync(d.gls_queue, 0, kGlsQueueInts * sizeof(int32_t), stream));   // the launches' work counters
            const int only = gls_only();
            if (only < 0) rc = gls_side_begin(d, -1, add_neumann, dev_csr_data, dev_neumann_ws, stream);
            if (!rc) rc = gls_main(d, -1, true, only, add_neumann, dev_csr_data, dev_neumann_ws, stream);
        }
        if (rc) return rc;
        return NIN_OK;
    }
    // explicit target list: outputs of every other node are zero
    for (int64_t i = 0; i < n_targets; ++i)
        if (targets[i] < 0 || targets[i] >= P) return fail(NIN_EINVAL, "target %lld out of range", (long long)targets[i]);
    HIP_TRY(hipMemsetAsync(dev_csr_data, 0, (size_t)d.nnz_e * 8, stream));
    HIP_TRY(hipMemsetAsync(dev_neumann_ws, 0, (size_t)P * 8, stream));
    if (n_targets == 0) return NIN_OK;
    const bool gls = method == NIN_METHOD_GLS;
    std::vector<int32_t> lists[kGlsPlanKernels];   // the targets by plan kernel (IDW / LS: all in the first)
    for (int64_t i = 0; i < n_targets; ++i) lists[gls ? gls_class_kernel(g->node_class[targets[i]]) : 0].push_back((int32_t)targets[i]);
    // one device buffer for all lists and their descriptors, filled before the first launch: a per-list allocate / copy / free
    // cycle lets the allocator hand the same memory to the next list while the previous kernel still reads it
    // (the pageable copy is not ordered behind that kernel)
    std::vector<int32_t> flat;
    int32_t off[kGlsPlanKernels + 1];                      // where a list begins
    size_t desc_first[kGlsPlanKernels], words = 0;         // where its descriptors begin, behind the lists
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        off[k] = (int32_t)flat.size();
        desc_first[k] = words = desc_align(words);
        flat.insert(flat.end(), lists[k].begin(), lists[k].end());
        if (gls) words += lists[k].size() * (size_t)gls_plan_row(k).desc_words;
    }
    off[kGlsPlanKernels] = (int32_t)flat.size();
    const size_t list_words = desc_align(flat.size());     // (the descriptors begin on a 16-byte boundary)
    DevTmp<int32_t> dl0;
    HIP_TRY(hipMalloc((void **)&dl0, (list_words + words) * 4));
    const hipError_t e = hipMemcpy(dl0, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(NIN_EHIP, "hipMemcpy: %s", hipGetErrorString(e));
    rc = launch_lists(d, method, dl0, off, reinterpret_cast<uint32_t *>(dl0 + list_words), desc_first, add_neumann, dev_csr_data,
                      dev_neumann_ws, stream, nullptr);
    const hipError_t sy = hipStreamSynchronize(stream);   // the lists must outlive the kernels: dl0 goes after this
    if (sy != hipSuccess) return fail(NIN_EHIP, "target kernels: %s", hipGetErrorString(sy));
    return rc;
}

int nin_weights_host(nin_grid *g, int method, const int64_t *targets, int64_t n_targets, int add_neumann,
                     double *csr_data, double *neumann_ws) {
    if (!g || !csr_data || !neumann_ws) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    if (int rc = on_device(g, kHintWeights, false)) return rc;
    HIP_TRY(hipSetDevice(d.device));
    const size_t nb = (size_t)std::max<int64_t>(d.nnz_e, 1) * 8, pb = (size_t)g->h.n_points * 8;
    DevTmp<double> dd, dn;
    HIP_TRY(hipMalloc((void **)&dd, nb));
    hipError_t e = hipMalloc((void **)&dn, pb);
    if (e != hipSuccess) return fail(NIN_ENOMEM, "hipMalloc: %s", hipGetErrorString(e));
    int rc = nin_weights_device(g, method, targets, n_targets, add_neumann, dd, dn, nullptr);
    if (!rc) {
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(csr_data, dd, (size_t)d.nnz_e * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(neumann_ws, dn, pb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(NIN_EHIP, "weights kernel / copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

// ---- algorithmic flops of a launch plan, kernel by kernel (tools/count_algorithmic_flops.py holds the same formulas) ----
namespace {
// n_pivot Householder steps on an m-row block with n_cols columns in all (pivot columns included): 2 m for the norm, 8 for the
// scalar chain, 4 m per trailing column (dot + update)
double hh_flops(int64_t m, int64_t n_pivot, int64_t n_cols) {
    double f = 0;
    for (int64_t k = 0; k < n_pivot; ++k) {
        const double rows = (double)(m - k);
        f += 2 * rows + 8 + 4 * rows * (double)(n_cols - k - 1);
    }
    return f;
}
// fronts of 3-face cells + a dense rest (kernels_gls_hex8mf / mfw / mfx): F fronts, D dense cells, `faces` internal faces of which
// `free_faces` join two dense cells
double multifrontal_flops(int64_t F, int64_t D, int64_t faces, int64_t free_faces, int64_t neumann_rows = 0) {
    const double face = 52.0 * faces + 15.0 * neumann_rows;
    const double p1 = F * (hh_flops(10, 3, 3 + 9 + 1) + 9 + 54 + 6);
    const int64_t m2 = 7 * F + D + 3 * free_faces + neumann_rows, n2 = 3 * D;
    const double p2 = hh_flops(m2, n2, n2 + 1);
    const double tail = (double)n2 * n2 + F * (2 * 9 + 2) + D * (2 * 3 + 1) + 2 * (m2 - n2) + (F + D) + 1;
    return face + p1 + p2 + tail;
}
// the dense m x (n + 1) system with the last-row identity (one Householder QR of the first n columns, no right-hand sides):
// the small-node, block (one wavefront) and global-scratch kernels; n_if internal faces, n_nb Neumann rows
double dense_flops(int64_t ne, int64_t n_if, int64_t n_nb) {
    const int64_t m = ne + 3 * n_if + n_nb, n = 3 * ne;
    return 52.0 * n_if + 15.0 * n_nb + hh_flops(m, n, n + 1) + (double)n * n + 7.0 * ne + 2.0 * (m - n) + ne + 1;
}
// dgels on the reference's dense m x n system with nrhs right-hand sides
double dgels_flops(double m, double n, double nrhs) { return 2 * m * n * n - 2 * n * n * n / 3 + nrhs * (4 * m * n - 2 * n * n) + nrhs * n * n; }
}  // namespace

int nin_gls_plan_flops(nin_grid *g, double alg[22], double ref[22], int64_t computed[22]) {
    if (!g || !alg || !ref || !computed) return fail(NIN_EINVAL, "NULL argument");
    DeviceGrid &d = g->d;
    HostGrid &h = g->h;
    if (int rc = on_device(g, kHintToDevice)) return rc;
    if (!d.fields_set || (!d.flag_staging && !d.flags_host_stale))
        return fail(NIN_ESTATE, "nin_fields_set has not been called (the Neumann flags decide which boundary nodes are computed)");
    if (h.ensure(A_ESUP_PTR | A_ESUP | A_FSUP_PTR | A_FSUP | A_ESUF)) return fail(NIN_EHIP, "mirroring the connectivity failed");
    HIP_TRY(hipSetDevice(d.device));
    {   // after an update of the flags from device memory the host's copy of the bytes is fetched again (waits for the device)
        const int frc = fetch_flag_bytes(g);
        if (frc) return frc;
    }
    for (int k = 0; k < kGlsPlanKernels; ++k) { alg[k] = ref[k] = 0.0; computed[k] = 0; }
    const int64_t P = h.n_points;
    // (F, D, free faces) of the nodes of the multifrontal kernels: the low 24 bits of the descriptor word the plan's table names
    std::vector<uint32_t> fdq((size_t)P, 0u);
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        const GlsPlanRow row = gls_plan_row(k);
        const auto &l = d.plan[k];
        if (row.fdq_word < 0 || l.count <= 0) continue;
        std::vector<int32_t> hn((size_t)l.count);
        std::vector<uint32_t> hd((size_t)l.count * row.desc_words);
        if (hipMemcpy(hn.data(), l.nodes, hn.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hd.data(), l.desc, hd.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(NIN_EHIP, "reading the descriptors back failed");
        for (int32_t i = 0; i < l.count; ++i) fdq[hn[i]] = hd[(size_t)i * row.desc_words + row.fdq_word] & 0xFFFFFFu;
    }
    for (int64_t p = 0; p < P; ++p) {
        const int k = gls_class_kernel(g->node_class[p]);
        const GlsPlanRow row = gls_plan_row(k);
        const int fl = d.flag_staging[p];
        if ((fl & 1) && !(fl & 2)) continue;                   // a Dirichlet boundary node: the zero row, nothing computed (gls.pyx:165-166)
        const int64_t eb = h.esup_ptr[p], ne = h.esup_ptr[p + 1] - eb, fb = h.fsup_ptr[p], nf = h.fsup_ptr[p + 1] - fb;
        int64_t n_if = 0;
        for (int64_t q = fb; q < fb + nf; ++q) {
            const int64_t f = h.fsup[q];
            n_if += h.esuf_ptr[f + 1] - h.esuf_ptr[f] > 1;
        }
        const int64_t n_bf = nf - n_if, n_nb = (fl & 2) ? n_bf : 0;
        const int64_t m = ne + 3 * n_if + n_nb;
        if (n_if == 0 || m < 3 * ne) continue;                 // outside the parity set: the zero row
        ++computed[k];
        ref[k] += dgels_flops((double)(ne + 3 * nf + n_nb), (double)(3 * ne + 1), (double)(ne + (n_nb ? 1 : 0)));
        if (k == gk::hex8) alg[k] += multifrontal_flops(4, 4, 12, 0);
        else if (row.fdq_word >= 0) {   // the multifrontal kernels with descriptors; all but the one-wavefront kernel take Neumann rows
            const uint32_t w = fdq[p];
            alg[k] += multifrontal_flops(w & 255u, (w >> 8) & 255u, n_if, (w >> 16) & 255u, row.family != GlsFamily::mfw ? n_nb : 0);
        } else if (k == gk::quad4) {
            // two fronts of 8 rows (cell row, two internal faces, the Neumann row) x (3 | 6 | c), then 14 x 6 over the pair
            alg[k] += 52.0 * 4 + 15.0 * 4 + 2 * (hh_flops(8, 3, 3 + 6 + 1) + 9 + 36 + 6) + hh_flops(14, 6, 7) + 36 + 2 * 20 + 2 * 7 + 2 * 8 + 5;
        } else if (k >= gk::block2 && k <= gk::block8) {
            // the block kernel on more than one wavefront: fronts = the greedy independent set (esup order) of the cells with 1 .. 4
            // internal faces at the node that own no Neumann row; a front of a cell with f faces is (1 + 3 f) x (3 + 3 f + 1)
            const int n_c = (int)std::min<int64_t>(ne, 64);
            uint64_t adj[64] = {0};
            int nfi[64] = {0};
            uint64_t blocked = 0;
            for (int64_t q = fb; q < fb + nf; ++q) {
                const int64_t f = h.fsup[q], e0 = h.esuf_ptr[f];
                const bool internal = h.esuf_ptr[f + 1] - e0 > 1;
                int ia = -1, ib = -1;
                for (int i = 0; i < n_c; ++i) {
                    if (h.esup[eb + i] == h.esuf[e0]) ia = i;
                    if (internal && h.esup[eb + i] == h.esuf[e0 + 1]) ib = i;
                }
                if (internal && ia >= 0 && ib >= 0) { adj[ia] |= 1ull << ib; adj[ib] |= 1ull << ia; ++nfi[ia]; ++nfi[ib]; }
                else if (!internal && ia >= 0 && n_nb) blocked |= 1ull << ia;
            }
            uint64_t chosen = 0;
            double p1 = 0;
            int64_t rows_gone = 0, Fb = 0;
            for (int i = 0; i < n_c; ++i)
                if (nfi[i] >= 1 && nfi[i] <= 4 && !((blocked >> i) & 1ull) && !(adj[i] & chosen)) {
                    chosen |= 1ull << i;
                    p1 += hh_flops(1 + 3 * nfi[i], 3, 3 + 3 * nfi[i] + 1);
                    rows_gone += 3;
                    ++Fb;
                }
            const int64_t m2 = m - rows_gone, n2 = 3 * (ne - Fb);
            alg[k] += 52.0 * n_if + 15.0 * n_nb + p1 + hh_flops(m2, n2, n2 + 1) + (double)(3 * ne) * (3 * ne) + 7.0 * ne + 2.0 * (m - 3 * ne) + ne + 1;
        } else {
            alg[k] += dense_flops(ne, n_if, n_nb);             // small-node kernel, block kernel on one wavefront, global scratch
        }
    }
    return NIN_OK;
}

int nin_gls_plan(const nin_grid *g, int64_t counts[22]) {
    if (!g || !counts) return fail(NIN_EINVAL, "NULL argument");
    if (int rc = on_device(g, kHintToDevice)) return rc;
    for (int k = 0; k < kGlsPlanKernels; ++k) counts[k] = g->d.plan[k].count;
    return NIN_OK;
}
