// The constants and records that the index tables of a problem share with the kernels that walk them: plain C++, no HIP header
// (csrc/kernels.h includes this file; host/problem_plan.cpp builds the tables with nothing else).
#pragma once
#include <stdint.h>

namespace aar {

constexpr int CHOL_NB = 96;       // dense LDL^T tile (16 entity blocks of 6)
constexpr int PASSB_CHUNK = 1024;  // upper limit of AAR_PASSB_CHUNK (observations of one (camera, marker) run handled by one wavefront; the default rule stops at 512)

// Per-observation record of an ordering: {frame (local), camera, marker, frame-local W slots: camera | marker << 10 | intrinsics << 21}
struct ObsIdx {
    int32_t frame, cam, marker, slots;
};

constexpr int SLOT_C_BITS = 10, SLOT_M_BITS = 11;   // ObsIdx::slots
inline int pack_slots(int sc, int sm, int sk) { return sc | (sm << SLOT_C_BITS) | (sk << (SLOT_C_BITS + SLOT_M_BITS)); }

}  // namespace aar
