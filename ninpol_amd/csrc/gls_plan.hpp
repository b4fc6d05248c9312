// gls_plan.hpp -- the GLS launch plan: the one place that knows which kernels there are (internal).
//
// A node is given to exactly one GLS kernel when the grid goes to the device (grid_device.hip: k_classify writes one class byte per
// node).  Everything the host needs to route a node -- the kernel's public index, its launcher family, the class byte, the size of its
// descriptors, its work counter -- is one row of gls_plan_row() below.  A new kernel costs one enumerator, one row, one case in
// abi_plan.hip's launch_plan_kernel and, if it has descriptors, one in launch_plan_desc.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define NIN_HD __host__ __device__
#else
#define NIN_HD
#endif

namespace nin {

constexpr int kGlsClasses = 5;  // four LDS budget classes (1 / 2 / 4 / 8 waves per node) + one global-scratch class

// The kernels of the plan in their PUBLIC order: index k of nin_gls_plan / nin_gls_plan_flops (include/ninpol_amd.h), of
// Grid.PLAN_KERNELS (grid.py: the same names) and of NIN_GLS_ONLY=<k>.  (mfx_4x7 and mfx_7x12 came after mfg_tiles had taken 19.)
constexpr int kGlsPlanKernels = 22;
namespace gk {   // (a namespace of their own: gk::scratch, not a name a local variable can hide)
enum GlsKernel : int {
    block1, block2, block4, block8, scratch,
    hex8,
    mfw_large, mfw_small, mfw_general,
    small4, small8, small12,
    quad4,
    mfx_6x10, mfx_7x11, mfx_8x13, mfx_9x15, mfx_10x16,
    mfx_boundary,
    mfg_tiles,
    mfx_4x7,
    mfx_7x12,
};
}  // namespace gk
using gk::GlsKernel;

// which launcher takes the list (abi_plan.hip: launch_plan_kernel / launch_plan_desc switch over this)
enum class GlsFamily : uint8_t {
    block,    // kernels_gls_block.hip: one node per workgroup, system in LDS; sub = the LDS class
    scratch,  // kernels_gls.hip: the wave kernel on global-memory scratch
    hex8,     // kernels_gls_hex8mf.hip: cube nodes
    mfw,      // kernels_gls_mfw.hip: the one-wavefront multifrontal kernel; sub = kind
    small,    // kernels_gls_mfw.hip, nin_gls_small_kernel; sub = kind (at most 4 / 8 / 12 cells)
    quad4,    // kernels_gls_quad4.hip: nodes inside a boundary face of a hexahedron mesh
    mfx,      // kernels_gls_mfx.hip: the wide multifrontal kernel; sub = list = the kernel's size-class argument
    mfg,      // kernels_gls_mfg.hip: the multifrontal kernel on global-memory tiles
};

// The GLS kernels' work counters: one block of kGlsQueueInts ints per grid (DeviceGrid::gls_queue), zeroed before every launch (and
// before every piece of interpolate()'s pipeline).  The kernels of one launch run at the same time -- the side stream's under the main
// stream's -- so no two of them may share an int:
//   hex8       ints 0 + 16 * xcd   one per XCD, each on its own 64-byte line (a grid of fewer than 8 workgroups uses int 0 alone)
//   block      ints 1 .. 4         one per LDS class
//   mfw        ints 5 .. 7         one per kind
//   mfx        ints 8 .. 15        one per list
//   mfg        int 128             a 64-byte line of its own, past hex8's eight
constexpr int kGlsQueueLine = 16;                 // ints per 64-byte line
constexpr int kGlsQueueHex8 = 0, kGlsQueueHex8Lines = 8;
constexpr int kGlsQueueBlock = 1;                 // + class (0 .. kGlsClasses - 2)
constexpr int kGlsQueueMfw = 5;                   // + kind (0 .. 2)
constexpr int kGlsQueueMfx = 8, kGlsQueueMfxLists = 8;   // + list
constexpr int kGlsQueueMfg = 8 * kGlsQueueLine;
constexpr int kGlsQueueInts = 9 * kGlsQueueLine;
static_assert(kGlsQueueBlock > kGlsQueueHex8 && kGlsQueueBlock + (kGlsClasses - 1) <= kGlsQueueMfw, "block counters overlap");
static_assert(kGlsQueueMfw + 3 <= kGlsQueueMfx, "mfw counters overlap the mfx counters");
static_assert(kGlsQueueMfx + kGlsQueueMfxLists <= kGlsQueueLine, "the block / mfw / mfx counters must stay between hex8's ints 0 and 16");
static_assert(kGlsQueueMfg % kGlsQueueLine == 0 && kGlsQueueMfg / kGlsQueueLine >= kGlsQueueHex8 / kGlsQueueLine + kGlsQueueHex8Lines,
              "the mfg counter must lie on none of hex8's eight lines");
static_assert(kGlsQueueMfg < kGlsQueueInts, "the mfg counter lies outside the block");

struct GlsPlanRow {
    GlsFamily family;
    int8_t sub;           // the kind / class / list argument of the family's launcher
    uint8_t class_byte;   // what k_classify writes for a node of this kernel
    int16_t desc_words;   // descriptor words per list entry (hex8_desc / quad4_desc / mfw_desc / mfx_desc / mfg_desc.hpp), 0: none
    int16_t fdq_word;     // the descriptor word whose low 24 bits are (F, D, free faces), for nin_gls_plan_flops; -1: none
    int16_t counter;      // the kernel's work counter: an offset into gls_queue; -1: the kernel takes none
};
// (the descriptor sizes are mfw_desc / mfx_desc / mfg_desc.hpp's kM*DescWords: those headers include this one, abi_plan.hip asserts the match)
constexpr int kGlsDescHex8 = 32, kGlsDescQuad4 = 2, kGlsDescMfw = 40, kGlsDescMfx = 56, kGlsDescMfg = 124;

NIN_HD constexpr GlsPlanRow gls_plan_row(int k) {
    using F = GlsFamily;
    constexpr GlsPlanRow rows[kGlsPlanKernels] = {
        // family   sub  byte  desc words     fdq  counter
        {F::block,   0,    0,  0,             -1,  kGlsQueueBlock + 0},   // block1
        {F::block,   1,    1,  0,             -1,  kGlsQueueBlock + 1},   // block2
        {F::block,   2,    2,  0,             -1,  kGlsQueueBlock + 2},   // block4
        {F::block,   3,    3,  0,             -1,  kGlsQueueBlock + 3},   // block8
        {F::scratch, 4,    4,  0,             -1,  -1},                   // scratch
        {F::hex8,    0,  255,  kGlsDescHex8,  -1,  kGlsQueueHex8},        // hex8
        {F::mfw,     0,  254,  kGlsDescMfw,   24,  kGlsQueueMfw + 0},     // mfw_large
        {F::mfw,     1,  253,  kGlsDescMfw,   24,  kGlsQueueMfw + 1},     // mfw_small
        {F::mfw,     2,  252,  kGlsDescMfw,   24,  kGlsQueueMfw + 2},     // mfw_general
        {F::small,   0,  249,  0,             -1,  -1},                   // small4
        {F::small,   1,  250,  0,             -1,  -1},                   // small8
        {F::small,   2,  251,  0,             -1,  -1},                   // small12
        {F::quad4,   0,  248,  kGlsDescQuad4, -1,  -1},                   // quad4
        {F::mfx,     0,  243,  kGlsDescMfx,    0,  kGlsQueueMfx + 0},     // mfx_6x10
        {F::mfx,     1,  244,  kGlsDescMfx,    0,  kGlsQueueMfx + 1},     // mfx_7x11
        {F::mfx,     2,  245,  kGlsDescMfx,    0,  kGlsQueueMfx + 2},     // mfx_8x13
        {F::mfx,     3,  246,  kGlsDescMfx,    0,  kGlsQueueMfx + 3},     // mfx_9x15
        {F::mfx,     4,  247,  kGlsDescMfx,    0,  kGlsQueueMfx + 4},     // mfx_10x16
        {F::mfx,     5,  242,  kGlsDescMfx,    0,  kGlsQueueMfx + 5},     // mfx_boundary
        {F::mfg,     0,  241,  kGlsDescMfg,    0,  kGlsQueueMfg},         // mfg_tiles
        {F::mfx,     6,  240,  kGlsDescMfx,    0,  kGlsQueueMfx + 6},     // mfx_4x7
        {F::mfx,     7,  239,  kGlsDescMfx,    0,  kGlsQueueMfx + 7},     // mfx_7x12
    };
    return rows[k];
}

// kernel -> class byte and back (-1: no kernel has that byte)
NIN_HD constexpr uint8_t gls_class_byte(GlsKernel k) { return gls_plan_row(k).class_byte; }
NIN_HD constexpr int gls_class_kernel(int class_byte) {
    for (int k = 0; k < kGlsPlanKernels; ++k)
        if (gls_plan_row(k).class_byte == class_byte) return k;
    return -1;
}

// The routing switches k_classify receives as one int (`use_group`): nin_grid_to_device sets a bit unless (*: if) the environment
// variable is there
enum GlsRoute : int {
    kRouteHex8 = 1,              // NIN_GLS_NO_GROUP: keep nodes away from the cube-node kernel
    kRouteMfw = 2,               // NIN_GLS_NO_MFW: ... from the one-wavefront multifrontal kernel
    kRouteMfwGeneral = 4,        // NIN_GLS_NO_MFW_GENERAL: ... from its general kind
    kRouteSmall = 8,             // NIN_GLS_NO_SMALL: ... from the one-wavefront dense kernel for small nodes
    kRouteQuad4 = 16,            // NIN_GLS_NO_QUAD4: ... from the two-lanes-per-node kernel for quad nodes
    kRouteMfx = 32,              // NIN_GLS_NO_MFX: ... from the wide multifrontal kernel (unstructured meshes)
    kRouteMfxTakesGeneral = 64,  // NIN_GLS_MFW_GENERAL clears it: the wide kernel takes the general kind's nodes that fit it too -- the default since
                                 // its dense phase runs straight-line per size class (37 against 38 ns a node on a Delaunay mesh, equal on the mixed mesh)
    kRouteMfxNoBoundary = 128,   // * NIN_GLS_MFX_NO_BOUNDARY: the wide kernel leaves the boundary nodes to the block kernel (round 3's route)
    kRouteMfg = 256,             // NIN_GLS_NO_MFG: ... from the multifrontal kernel on global-memory tiles (nodes beyond the wide kernel)
    kRouteMfxSmall = 512,        // NIN_GLS_NO_MFX_SMALL: ... from the wide kernel's small class (4, 7) for interior nodes of 9 .. 14 cells
    kRouteMfx7x12 = 1024,        // NIN_GLS_NO_MFX_7X12: ... from its class (7, 12)
};

// ---- what a reviewer would otherwise have to check by eye ----
static_assert(gk::block1 == 0 && gk::scratch == 4 && gk::hex8 == 5 && gk::mfw_large == 6 && gk::mfw_general == 8 && gk::small4 == 9 &&
                  gk::small12 == 11 && gk::quad4 == 12 && gk::mfx_6x10 == 13 && gk::mfx_10x16 == 17 && gk::mfx_boundary == 18 &&
                  gk::mfg_tiles == 19 && gk::mfx_4x7 == 20 && gk::mfx_7x12 == 21 && gk::mfx_7x12 + 1 == kGlsPlanKernels,
              "GlsKernel must keep the public numbering of include/ninpol_amd.h");
// the block kernel's classes and the scratch class are what gls_node_class() returns: kernel == class byte == sub, 0 .. kGlsClasses - 1;
// every other byte lies above them and belongs to one kernel only
constexpr bool plan_class_bytes_ok() {
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        const GlsPlanRow r = gls_plan_row(k);
        const bool sized = r.family == GlsFamily::block || r.family == GlsFamily::scratch;
        if (sized != (k < kGlsClasses) || (sized && (r.class_byte != k || r.sub != k)) || (!sized && r.class_byte < kGlsClasses)) return false;
        for (int j = 0; j < k; ++j)
            if (gls_plan_row(j).class_byte == r.class_byte) return false;
    }
    // (k_classify computes the byte of the wide kernel's size classes from mfx_descriptor's code and the first of them)
    for (int i = 0; i < 5; ++i)
        if (gls_class_byte(GlsKernel(gk::mfx_6x10 + i)) != gls_class_byte(gk::mfx_6x10) + i || gls_plan_row(gk::mfx_6x10 + i).sub != i) return false;
    return true;
}
// does kernel k's work counter take int i?  (hex8: one per line on kGlsQueueHex8Lines lines; every other kernel: one)
constexpr bool plan_takes_int(int k, int i) {
    const GlsPlanRow r = gls_plan_row(k);
    if (r.counter < 0 || r.family != GlsFamily::hex8) return r.counter >= 0 && i == r.counter;
    return i >= r.counter && (i - r.counter) % kGlsQueueLine == 0 && (i - r.counter) / kGlsQueueLine < kGlsQueueHex8Lines;
}
// all kernels of the plan can run in one launch: no int is taken twice, and none lies outside the block
constexpr bool plan_counters_ok() {
    for (int k = 0; k < kGlsPlanKernels; ++k) {
        const GlsPlanRow a = gls_plan_row(k);
        if (a.counter + (a.family == GlsFamily::hex8 ? kGlsQueueHex8Lines - 1 : 0) * kGlsQueueLine >= kGlsQueueInts) return false;
        for (int j = 0; j < kGlsPlanKernels; ++j)   // (k's first int against all of j's: a later line of hex8's is met when the other kernel is k)
            if (j != k && a.counter >= 0 && plan_takes_int(j, a.counter)) return false;
    }
    return true;
}
static_assert(plan_class_bytes_ok(), "class bytes: 0 .. 4 for the block / scratch classes, distinct and above 4 for every other kernel, mfx_6x10 .. mfx_10x16 in a row");
static_assert(plan_counters_ok(), "two kernels of the plan share a work counter, or one lies outside gls_queue");

}  // namespace nin
