// frt-mi355x scene-specialised shadow kernel (frt_jit.hip): host interface used by the engine.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "frt_knobs.hpp"

namespace frt {
struct WalkNode;
}
struct frt_light;

// The stage sizes are upload knobs (frt_knobs.hpp): PS = jit_part samples per light part of the pair kernels, the tile
// kernel's jit_tile consecutive path nodes, the sub-part pass's Q = jit_sub sub-parts per part, the sub-tile kernel's
// jit_subtile nodes. The sub-parts' sizes, the largest (PS2), and the sub-parts' samples:
std::vector<int> frt_jit_sub_sizes(int c, int Q);
int frt_jit_sub_ps(int PS, int Q);
int frt_jit_light_subparts(const frt_light& L, const double* light_points, const std::vector<int32_t>& order, int PS,
                           int Q, std::vector<int32_t>& order2);
// the nodes per super-tile these knobs give (jit_supertile where it exceeds the tile size and the tile and sub-part
// stages are on), else 0: no split kernel, the lists' entries by tile
inline int frt_jit_supertile(const UploadKnobs& K) {
    return K.jit_tile > 0 && K.jit_sub > 0 && K.jit_supertile > K.jit_tile ? K.jit_supertile : 0;
}
// the parts (frt_jit.hip): spatially compact groups of the light's samples; returns the part count
int frt_jit_light_parts(const frt_light& L, const double* light_points, int PS, std::vector<int32_t>& order);

// HIP source of the shadow kernel for this tree and these lights ("" and `why` set when the scene
// is not eligible: too many nodes, or a CSG unit with a leaf whose list is unsorted)
std::string frt_jit_shadow_source(const frt::WalkNode* wn, int num_nodes, const int32_t* roots, int num_roots,
                                  const frt_light* lights, int num_lights, const UploadKnobs& K, std::string& why);

// the kernels of a scene's module (hipFunction_t; tile / list are null when the source has none)
struct FrtJitFns {
    void* shadow = nullptr;  // frt_jit_shadow: per ray
    void* beam = nullptr;    // frt_jit_beam: every (node, part) pair
    void* tile = nullptr;    // frt_jit_tile: every (tile, part) pair
    void* list = nullptr;    // frt_jit_beam_list: the nodes of the listed tile pairs
    void* sub = nullptr;     // frt_jit_sub: the sub-parts of the tile pairs left mixed
    void* subtile = nullptr; // frt_jit_subtile: the sub-tiles of the tile sub-pairs left mixed
    void* split = nullptr;   // frt_jit_split: the tiles of the (super-tile, sample) pairs left mixed
    void* trace = nullptr;   // frt_jit_trace: closest hit per ray (null where the scene has none)
};
// compile with hiprtc for `device` (cached per device and source); 0 on success
int frt_jit_compile(const std::string& src, int device, const UploadKnobs& K, FrtJitFns& fns, std::string& log);

// this thread's last frt_jit_compile: ms to obtain the code object (0 when the process had it; a disk
// read or a hiprtc compile otherwise) and to load it into the device's module
void frt_jit_last_phases(double* obtain_ms, double* load_ms);

// compile only (no device needed): 0 on success
int frt_jit_compile_only(const std::string& src, const std::string& arch, const UploadKnobs& K, std::string& log);
