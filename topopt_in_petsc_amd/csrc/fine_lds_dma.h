// fine_lds_dma.h -- the LDS-DMA staging that the third generation of the fine-level operator (fine_u4.h) is built on: the
// LDS map of a tile, the DMA and wait primitives, and the 16-byte staging windows.  (matfree_tile.h holds the
// mathematics, fine_tile.h the second generation and the measurements that led here.)
//
// What round 2 measured: at 256^3 the data-movement skeleton of k_fine_tile runs at 0.40 of the HBM peak
// and the time does not follow the bytes (z-chunks of 16 or 129 planes: the same 328 us).  Each workgroup has exactly
// ONE step of loads in flight (4 x 8 B per lane held in VGPRs): a step costs one loaded memory round trip, whatever it
// computes.  More bytes in flight need either registers (there are none left at 3 waves per SIMD) or LDS:
//
//  * node planes and the moduli reach LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`: 16 B per lane, no VGPR, no
//    ds_write), D steps ahead, into rings of slots.  A tile row is ONE contiguous run
//    of 16-byte units that starts at the 16-byte boundary at or below its first node: the units of a wave instruction
//    land lane-linear, so the LDS image of a row is [parity pad][nodes ...] and the reader adds the row's parity.
//  * every vector-memory instruction of the loop is issued by hand (inline asm) in a fixed order and count per step, and
//    the waits are counted by hand: the compiler's own s_waitcnt insertion does not know LDS-DMA and would drain the
//    queue at the first ordinary load (cdna_hip_programming.md, "Pipelining across barriers").  Order per step:
//        [top]  batch(s) = planes' units, moduli units          (needed by step s + D)
//        [mid]  s_waitcnt vmcnt((D-1) * OPS) -> batch(s+1-D) has landed for THIS wave; the step's barrier publishes it
//        [end]  epilogue operands of step s+1 (b, u-: VGPR loads), then the stores of step s
//    The prologue issues the same pattern (stores and operand loads against empty descriptors: counted, no traffic) so
//    that one immediate fits every step.  Out-of-range planes and everything beyond the last plane a chunk needs are
//    requested through an EMPTY descriptor: zeros in LDS, no memory traffic (the second generation fetched two planes
//    per chunk that nobody read).
//  * the tile shape is a template parameter: TX lanes along x (16: DPP row shift, 32/64: DPP wave shift), TY rows.
//
// Per-node arithmetic and summation order are those of k_fine_tile: results are bitwise identical to it.
// (The first kernel on this scheme, k_fine_dma with its ring depth D as a template parameter, measured what fine_u4.h
// starts from; it was never launched by the library and is gone -- DESIGN_HISTORY.md, round 3.)
#pragma once
#include <type_traits>

#include "fine_tile.h"

template <int TX, int TY, int D>
struct FineDma {
    static constexpr int NT = TX * TY, NW = NT / 64;
    static constexpr int TOX = TX - 1, TOY = TY - 1;          // node columns / rows produced per tile
    static constexpr int UROWS = TY + 1, UPTS = TX + 1;        // staged node rows / nodes per row
    static constexpr int UPR_U = (3 * UPTS + 2) / 2;           // 16-byte units per staged node row (parity pad included)
    static constexpr int ROWW_U = 2 * UPR_U;                   // doubles per LDS row
    static constexpr int NUNIT_U = UROWS * UPR_U;
    static constexpr int NIU = (NUNIT_U + 63) / 64;            // wave instructions per plane
    static constexpr int NIU_W = (NIU + NW - 1) / NW;          // ... per wave
    static constexpr int USLOT = NIU * 1024;                   // bytes per ring slot
    static constexpr int UPR_E = (TX + 2) / 2;                 // units per staged modulus row
    static constexpr int ROWW_E = 2 * UPR_E;
    static constexpr int NUNIT_E = TY * UPR_E;
    static constexpr int NIE = (NUNIT_E + 63) / 64;
    static constexpr int NIE_W = (NIE + NW - 1) / NW;
    static constexpr int ESLOT = NIE * 1024;
    static constexpr int NI = NIU_W + NIE_W;                   // DMA instructions per wave and step
    static constexpr int RU = D + 2, RE = D + 1;               // ring depths
    static constexpr int MSZ = ((UROWS * UPTS + 15) / 16) * 16;  // mask bytes per plane (Dirichlet tiles)
    // LDS map (bytes)
    static constexpr int OFF_U = 0;
    static constexpr int OFF_E = OFF_U + RU * USLOT;
    static constexpr int OFF_Y = OFF_E + RE * ESLOT;
    static constexpr int YBUF = (NT - TX) * 3 * 8;             // y-combination buffer: the last row of a tile has no reader
    static constexpr int OFF_M = OFF_Y + 2 * YBUF;
    static constexpr int OFF_RED = OFF_Y;                      // block reduction of the dot epilogues (after the loop)
    static constexpr int LDS_BYTES = OFF_M + 4 * MSZ;
    static_assert(NT % 64 == 0, "whole waves");
    static_assert(TX == 16 || TX == 32 || TX == 64, "rows are 16, 32 or 64 lanes");
};

// left neighbour's value within the tile row (lanes with tx == 0 receive a value that is never used)
template <int TX>
__device__ __forceinline__ double dpp_left(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    if (TX == 16) {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xF, 0xF, true);  // row_shr:1
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xF, 0xF, true);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, true);  // wave_shr:1
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, true);
    }
    return __hiloint2double(hi, lo);
}

typedef double fd_d2 __attribute__((ext_vector_type(2)));
typedef unsigned fd_u4 __attribute__((ext_vector_type(4)));
typedef unsigned fd_u2 __attribute__((ext_vector_type(2)));
constexpr unsigned FD_RSRC_FLAGS = 0x00020000u;
constexpr unsigned FD_OOB = 0x80000000u;  // a voffset no descriptor of this file reaches (arrays < 2 GB, checked by the host)

// Hazards the compiler's recogniser does not see inside inline asm: an SGPR written by the SALU (or by v_readlane /
// v_readfirstlane: spilled descriptor words come back that way) needs 5 wait states before a vector-memory instruction
// reads it, otherwise the instruction may still see the OLD value -- a descriptor of the previous plane.  Every asm
// statement of this file that reads a descriptor therefore opens with its own wait states (the two s_mov + s_nop 2 of
// the DMA form, s_nop 4 elsewhere); the same s_nop covers the M0 write -> LDS-DMA hazard.
// one LDS-DMA wave instruction: 64 lanes x 16 B from rs[voff] to lds_dst + 16 * lane
__device__ __forceinline__ void fd_dma16(unsigned lds_dst, unsigned voff, __amdgpu_buffer_rsrc_t rs) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 2\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_dst), "v"(voff), "s"(rs)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void fd_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// voffset of a unit: stored value (rem = 0 offset, bit 0 = "the row's first double is odd") -> offset for this plane's rem.
// Offsets in front of the window (a tile's column -1 in the first row of a plane) are negative: every value >= 2^31 becomes
// FD_OOB exactly, which no descriptor of this file reaches (num_records <= 0x7FFFFF00) -> the hardware returns zeros.
__device__ __forceinline__ unsigned fd_voff(unsigned stored, int rem) {
    const unsigned v = (stored & ~1u) + (((stored & 1u) & (unsigned)rem) << 4);
    return v < FD_OOB ? v : FD_OOB;
}

// descriptor of the 16-byte-aligned window that starts at or below p; *rem = doubles between the window and p (0 | 1)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fd_window(const double *p, const double *end, bool on, int *rem) {
    const unsigned long a = (unsigned long)p;
    *rem = (int)((a >> 3) & 1ul);
    const unsigned long base = a & ~15ul;
    const long room = (long)((unsigned long)end - base);
    const int n = on ? (int)(room > 0x7FFFFF00l ? 0x7FFFFF00l : room) : 0;
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, n, FD_RSRC_FLAGS);
}
