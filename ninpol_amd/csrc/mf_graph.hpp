// mf_graph.hpp -- the packed descriptor layout that mfx_desc.hpp and mfg_desc.hpp share (internal, host and device code): the builders
// there write the words and kernels_gls_mfx.hip / kernels_gls_mfg.hip read them through one MfLayout each, so a field's offset, width
// and bit position have one definition.  The word layouts are documented at the top of the two headers.
#pragma once
#include <cstdint>

#include "device_grid.hpp"

namespace nin {

// One packed layout: word 0 = F | D << 8 | free << 16 | boundary << 24, then MAX_FRONTS words A (esup position of the front, 6 bits |
// fsup positions of its 3 faces, FACE_BITS each | SIDE_BIT + i: the front is face i's first cell), MAX_FRONTS words B (dense slots
// across the 3 faces, SLOT_BITS each), the slot table (esup position of dense slot d, one byte each) and from FREE0 the free faces
// (fsup position | slot of the first cell | slot of the second cell), behind them the boundary faces (fsup position | slot | bit 31).
template <int MAX_FRONTS, int MAX_DENSE, int MAX_FREE, int MAX_ROWS, int WORDS, int FREE0, int FACE_BITS, int SLOT_BITS, int SIDE_BIT>
struct MfLayout {
    static constexpr int MaxFronts = MAX_FRONTS, MaxDense = MAX_DENSE, MaxFree = MAX_FREE, MaxRows = MAX_ROWS, Words = WORDS;
    static constexpr int W0 = 1, W1 = 1 + MAX_FRONTS, SlotTable = 1 + 2 * MAX_FRONTS, Free0 = FREE0;
    static constexpr uint32_t FaceMask = (1u << FACE_BITS) - 1u, SlotMask = (1u << SLOT_BITS) - 1u;
    // word A / B of a front
    NIN_HD static uint32_t cell_pos(uint32_t wa) { return wa & 63u; }
    NIN_HD static uint32_t face_pos(uint32_t wa, int i) { return (wa >> (6 + FACE_BITS * i)) & FaceMask; }
    NIN_HD static bool side_a(uint32_t wa, int i) { return ((wa >> (SIDE_BIT + i)) & 1u) != 0; }
    NIN_HD static uint32_t slot(uint32_t wb, int i) { return (wb >> (SLOT_BITS * i)) & SlotMask; }
    NIN_HD static uint32_t pack_face(int fi, int k, bool a_front) { return ((uint32_t)fi << (6 + FACE_BITS * k)) | ((a_front ? 1u : 0u) << (SIDE_BIT + k)); }
    NIN_HD static uint32_t pack_slot(int slot, int k) { return (uint32_t)slot << (SLOT_BITS * k); }
    // the word of a free or boundary face
    NIN_HD static uint32_t free_pos(uint32_t fw) { return fw & FaceMask; }
    NIN_HD static uint32_t free_slot_a(uint32_t fw) { return (fw >> FACE_BITS) & SlotMask; }
    NIN_HD static uint32_t free_slot_b(uint32_t fw) { return (fw >> (FACE_BITS + SLOT_BITS)) & SlotMask; }
    NIN_HD static uint32_t pack_free(int fi, int sa, int sb) { return (uint32_t)fi | ((uint32_t)sa << FACE_BITS) | ((uint32_t)sb << (FACE_BITS + SLOT_BITS)); }
    NIN_HD static uint32_t pack_boundary(int fi, int sa) { return (uint32_t)fi | ((uint32_t)sa << FACE_BITS) | 0x80000000u; }
};

}  // namespace nin
