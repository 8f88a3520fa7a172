// frt-mi355x: every FRT_* environment knob of the engine, read here and nowhere else (host only).
//
// A knob has one of two lifetimes, and the struct it sits in says which:
//   UploadKnobs  read once by read_upload_knobs() at the top of frt_scene_upload (and of frt_jit_check, which has no
//                handle); kept in the handle. A change takes effect at the next upload.
//   FrameKnobs   read once by read_frame_knobs() at the top of each rendered frame (render_impl); kept in the handle.
//                A change takes effect at the next frame.
// Two diagnostics entry points have no handle either and call a reader at their top: frt_mesh_check
// (read_upload_knobs, for FRT_MESH) and frt_pm_estimate (read_frame_knobs, for the photon grid's FRT_PM_* knobs).
// FRT_JIT_TRACE has both: the upload decides whether frt_jit_trace is emitted, the frame whether it is used.
// FRT_WARMUP_* serve frt_device_warmup, which runs before any handle exists (read_warmup_knobs at its entry);
// FRT_WARMUP_TRACE also times the upload's stream creation and is therefore an upload knob as well.
//
// One row per knob: NAME  default  accepted values and clamping  meaning (with the A/B log where one was kept).
// "A/B" marks a knob that exists only to measure an alternative; the suite pins each mode by a bit-identity test.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

namespace frt_knobs {
inline const char* raw(const char* name) { return std::getenv(name); }
inline bool present(const char* name) { return raw(name) != nullptr; }
// on unless the value is the string "0"
inline bool unless_str0(const char* name) {
    const char* e = raw(name);
    return !(e && std::strcmp(e, "0") == 0);
}
// on unless the value is set and parses (atoi) to 0
inline bool unless_int0(const char* name) {
    const char* e = raw(name);
    return !(e && std::atoi(e) == 0);
}
inline int int_or(const char* name, int def) {
    const char* e = raw(name);
    return e ? std::atoi(e) : def;
}
inline long long ll_or(const char* name, long long def) {
    const char* e = raw(name);
    return e ? std::atoll(e) : def;
}
// the largest power of two <= x, at most 64; 0 for x < 2
inline int pow2_upto64(int x) {
    int p = 0;
    while (p < 6 && (2 << p) <= x) ++p;
    return x >= 2 ? 1 << p : 0;
}
// amdgpu_waves_per_eu requests: 1..8, anything else none (0)
inline int waves(const char* name) {
    const int n = int_or(name, 0);
    return n >= 1 && n <= 8 ? n : 0;
}
}  // namespace frt_knobs

struct UploadKnobs {
    // ---- which kernels an upload builds
    // FRT_JIT  on  "0" off  the scene-specialised shadow kernels (frt_jit.hip); off: the generic k_shadow
    bool jit = true;
    // FRT_JIT_BEAM  on  "0" off  the pair kernels; off: every pair is walked ray by ray (A/B)
    bool jit_beam = true;
    // FRT_JIT_NODE_BEAM  off  non-zero on  the (node, sample) pairs the sub-part / sub-tile stages leave are decided by
    //   frt_jit_beam_list one node beam per lane instead of walked by frt_jit_shadow directly (the default: a node's beam
    //   to one sample is one ray, and the per-ray walk costs a third of the beam walk's instructions; round 5,
    //   profiles/r05_ab_nodebeam.txt: headline 41.5 -> 36.4 ms, shipped light 90.5 -> 76.4 ms)
    bool jit_node_beam = false;
    // FRT_JIT_STATS  off  set: on  diagnostics counters in the generated kernels, printed at release
    bool jit_stats = false;
    // FRT_JIT_VERBOSE  off  set: on  says on stderr why a scene got the generic shadow walk
    bool jit_verbose = false;
    // FRT_JIT_DUMP  off  set: on  the generated source to stderr
    bool jit_dump = false;
    // FRT_JIT_TRACE (upload side)  on  0 off  emit the closest-hit kernel frt_jit_trace
    bool jit_trace = true;
    // FRT_MESH  on  "0" off  the mesh BVHs; off: the plain walk everywhere (A/B)
    bool mesh = true;
    // FRT_SHADE_SORT  on  0 off  the lit list in row order for the first multi-row area / circle light
    bool shade_sort = true;
    // FRT_SHADE_STAGE  2  any int  the row-ordered shading: 2 the node records read in row order, the triples written
    //   in row order (spos); 1 also the records staged in list order first (k_lit_stage); 0 both by node, as round 5
    //   did. Shipped frame: shade 14.2 / 13.1 / 12.9 ms for 0 / 1 / 2 (profiles/r06_ab_shipped_modes.txt)
    int shade_stage = 2;
    // FRT_QUEUE_SORT  2  any int  the secondary levels' queues read in parent order (reflected children, then
    //   refracted): appended to segment blockIdx % kQueueSegs, the segments' order put children of pixels 256 apart side
    //   by side, and the shadow pass's tiles of consecutive nodes spread over the scene. 2 the children at fixed slots
    //   (no queue atomics) compacted in order; 1 the segments' entries radix-sorted by parent; 0 the segments' order
    //   (A/B, profiles/r06_ab_queue_sort.txt)
    int queue_sort = 2;
    // FRT_QUEUE_SORT_SHIFT  0  clamped to 0..16  parents' low bits out of the sort key (A/B)
    int queue_sort_shift = 0;
    // FRT_PREPARE_UNIFORM  on  0 off  k_prepare: a wave whose lanes all hit one leaf reads that leaf's node, transforms
    //   and material through the scalar cache (frt_shade.hpp uniform_view); off: every wave per lane (A/B, tests)
    bool prepare_uniform = true;
    // FRT_WALK_FLAGS  0  any int  DevScene::walk_flags (A/B experiments only)
    int walk_flags = 0;

    // ---- the JIT source generator (frt_jit_shadow_source)
    // FRT_JIT_PART  16  1..1024, else 16  samples per light part of the pair kernels. 16 samples per part, split into
    //   single samples by the sub-part pass after the tile kernel (round 4, profiles/r04_ab_parts_tiles.txt,
    //   r04_ab_tile_sub.txt: with tiles and without the sub-part pass parts of 17 / 8 / 3 / 1 samples gave 95.2 / 88.3 /
    //   76.7 / 67.1 ms headline frames; 16 split in 16: 59.9 ms). Round 2, before the tile kernel, measured 17 best
    //   (profiles/r02_ab_parts_*.txt)
    int jit_part = 16;
    // FRT_JIT_TILE  64  rounded down to a power of two up to 64, below 2: 0 (off)  path nodes per tile of frt_jit_tile
    //   (a tile's nodes are consecutive lanes of one wave in k_prepare). 64: 59.9 ms headline frame with the sub-part
    //   pass, 32: 59.9; without it 64 beat 32 at every part size below 8 (profiles/r04_ab_parts_tiles.txt)
    int jit_tile = 64;
    // FRT_JIT_SUBTILE  16  rounded down to a power of two, below 2: 0 (off)  nodes per sub-tile of frt_jit_subtile, used
    //   where below the tile size (headline: off 60.8, 4 60.4, 8 57.1, 16 56.9, 32 57.6 ms; profiles/r04_ab_subtile.txt).
    //   Multi-row lights get no sub-tile kernel unless the knob is set at all (jit_subtile_set): the stage cut the
    //   shipped frame's per-ray lanes by 11 % for 6.5 ms; without it 76.4 -> 72.1 ms (profiles/r05_ab_nodebeam.txt)
    int jit_subtile = 16;
    bool jit_subtile_set = false;
    // FRT_JIT_SUB  16  2, 4, 8, 16 or 32, else 0 (off)  sub-parts per part of frt_jit_sub: the tile pairs left mixed are
    //   re-decided sample by sample (from the tile's origin box), so the node pair kernel only runs for the
    //   (tile, sample) pairs still mixed
    int jit_sub = 16;
    // FRT_JIT_SUPERTILE  512  128, 256, 512 or 1024, else 0 (off)  path nodes per super-tile: where it exceeds
    //   FRT_JIT_TILE and the sub-part stage is on, frt_jit_tile and frt_jit_sub decide runs of this many consecutive
    //   nodes (at level 0 adjacent pixels' samples) from the union of their tile boxes, and frt_jit_split re-decides
    //   the (super-tile, sample) pairs left per tile of the run before the sub-tile stage; ignored otherwise. A literal
    //   of the generated source (the split kernel's lanes, the later stages' entry decoding). Headline frame with every
    //   level on super-tiles, off / 128 / 256 / 512 / 1024: 27.00 / 25.13 / 24.16 / 23.97 / 23.91 ms; 1024 loses on
    //   cornell_direct_800_4x4 (2.79 -> 3.00 ms) and gains nothing on the shipped light (56.0 ms; 512: 54.4, 256: 54.2)
    //   (round 11, profiles/r11_ab_supertile.txt)
    int jit_supertile = 512;
    // FRT_JIT_INSIDE  on  0 off  the origin-inside shortcut for composite boxes (A/B)
    bool jit_inside = true;
    // FRT_JIT_U32  1  any int  0 bools everywhere, 1 32-bit decision values in the pair kernels' CSG units, 2 in the
    //   per-ray kernel's too (measured: the pair kernel 28.3 -> 26.5 ms per headline frame, the per-ray kernel
    //   54.8 -> 55.9 ms)
    int jit_u32 = 1;
    // FRT_JIT_ORDER  1  any int  same-axis slab order (jit::slab_order) in the tile kernel (1), in every pair kernel (2),
    //   or none (0). Measured on the headline: tile pairs mixed 77 -> 33 %, the node pairs left mixed the same (their
    //   undecided orders are between different axes' planes), the node pair kernel's time unchanged
    int jit_order = 1;
    // FRT_JIT_RESUME  on  0 off  the per-ray walk resumes from the pair kernel's resume point
    bool jit_resume = true;
    // FRT_JIT_FLAGS  on  0 off  entered-box flags in the resume value (A/B)
    bool jit_flags = true;
    // FRT_JIT_NODE_MAJOR  0 (unset: 4 for multi-row lights, 1 for single-row ones)  a power of two up to 64, else 1
    //   the per-ray kernel's lanes over the sub-part (sub-tile) stage's list, node-major over groups of this many
    //   entries (shipped frame: per-ray kernel 35.8 -> 32.4 ms at 4; 2 / 8 / 16 / 64: 35.7 / 32.8 / 33.5 / 38.1 ms,
    //   profiles/r06_ab_shipped_*.txt)
    int jit_node_major = 0;
    // FRT_JIT_RUN_COUNTS  on  0 off  off: one atomic per node and lit lane, as before round 6 (A/B)
    bool jit_run_counts = true;
    // FRT_JIT_DBG_NOWALK  0  any int  measurements only, wrong images: 1 the lanes' setup alone, 2 with the binary32 ray
    int jit_dbg_nowalk = 0;
    // FRT_JIT_TRACE_DBG  off  set: on, value = a ray index  debug: that lane's (and lane 0's) closest-hit walk, printed
    bool jit_trace_dbg = false;
    long long jit_trace_dbg_ray = 0;
    // FRT_JIT_WAVES / FRT_JIT_BEAM_WAVES / FRT_JIT_TRACE_WAVES  0  1..8, else 0  ask the compiler for at least n waves
    //   per SIMD in the per-ray / pair / closest-hit kernels (A/B)
    int jit_waves = 0, jit_beam_waves = 0, jit_trace_waves = 0;

    // ---- the JIT's code objects
    // FRT_JIT_CACHE ("0": no disk cache), FRT_JIT_CACHE_DIR, else $XDG_CACHE_HOME/frt_jit, else $HOME/.cache/frt_jit
    //   the directory of the on-disk code-object cache; empty: none
    std::string jit_cache_dir;
    // FRT_JIT_CO  unset  a path  diagnostics: keep the compiled code object there (llvm-objdump -d)
    std::string jit_co;

    // FRT_WARMUP_TRACE (upload side)  off  set: on  the upload's stream creation time to stderr
    bool warmup_trace = false;
};

inline UploadKnobs read_upload_knobs() {
    using namespace frt_knobs;
    UploadKnobs k;
    k.jit = unless_str0("FRT_JIT");
    k.jit_beam = unless_str0("FRT_JIT_BEAM");
    k.jit_node_beam = int_or("FRT_JIT_NODE_BEAM", 0) != 0;
    k.jit_stats = present("FRT_JIT_STATS");
    k.jit_verbose = present("FRT_JIT_VERBOSE");
    k.jit_dump = present("FRT_JIT_DUMP");
    k.jit_trace = unless_int0("FRT_JIT_TRACE");
    k.mesh = unless_str0("FRT_MESH");
    k.shade_sort = unless_int0("FRT_SHADE_SORT");
    k.shade_stage = int_or("FRT_SHADE_STAGE", 2);
    k.queue_sort = int_or("FRT_QUEUE_SORT", 2);
    k.queue_sort_shift = std::max(0, std::min(16, int_or("FRT_QUEUE_SORT_SHIFT", 0)));
    k.prepare_uniform = unless_int0("FRT_PREPARE_UNIFORM");
    k.walk_flags = int_or("FRT_WALK_FLAGS", 0);
    const int part = int_or("FRT_JIT_PART", 0);
    k.jit_part = part >= 1 && part <= 1024 ? part : 16;
    k.jit_tile = pow2_upto64(int_or("FRT_JIT_TILE", 64));
    k.jit_subtile = pow2_upto64(int_or("FRT_JIT_SUBTILE", 16));
    k.jit_subtile_set = present("FRT_JIT_SUBTILE");
    const int sub = int_or("FRT_JIT_SUB", 16);
    k.jit_sub = sub == 2 || sub == 4 || sub == 8 || sub == 16 || sub == 32 ? sub : 0;
    const int sup = int_or("FRT_JIT_SUPERTILE", 512);
    k.jit_supertile = sup == 128 || sup == 256 || sup == 512 || sup == 1024 ? sup : 0;
    k.jit_inside = unless_int0("FRT_JIT_INSIDE");
    k.jit_u32 = int_or("FRT_JIT_U32", 1);
    k.jit_order = int_or("FRT_JIT_ORDER", 1);
    k.jit_resume = unless_int0("FRT_JIT_RESUME");
    k.jit_flags = unless_int0("FRT_JIT_FLAGS");
    if (present("FRT_JIT_NODE_MAJOR")) {
        const int nm = int_or("FRT_JIT_NODE_MAJOR", 0);
        k.jit_node_major = nm >= 1 && nm <= 64 && (nm & (nm - 1)) == 0 ? nm : 1;
    }
    k.jit_run_counts = unless_int0("FRT_JIT_RUN_COUNTS");
    k.jit_dbg_nowalk = int_or("FRT_JIT_DBG_NOWALK", 0);
    k.jit_trace_dbg = present("FRT_JIT_TRACE_DBG");
    k.jit_trace_dbg_ray = ll_or("FRT_JIT_TRACE_DBG", 0);
    k.jit_waves = waves("FRT_JIT_WAVES");
    k.jit_beam_waves = waves("FRT_JIT_BEAM_WAVES");
    k.jit_trace_waves = waves("FRT_JIT_TRACE_WAVES");
    if (unless_str0("FRT_JIT_CACHE")) {
        if (const char* d = raw("FRT_JIT_CACHE_DIR")) k.jit_cache_dir = d;
        else if (const char* x = raw("XDG_CACHE_HOME")) k.jit_cache_dir = std::string(x) + "/frt_jit";
        else if (const char* home = raw("HOME")) k.jit_cache_dir = std::string(home) + "/.cache/frt_jit";
    }
    if (const char* co = raw("FRT_JIT_CO")) k.jit_co = co;
    k.warmup_trace = present("FRT_WARMUP_TRACE");
    return k;
}

struct FrameKnobs {
    // FRT_PRECISION  unset (parity)  "parity", "fast32", empty; anything else fails the frame with the value named
    //   the shading precision of a frame whose params name none (frame_precision)
    std::string precision;
    // FRT_BATCH_SAMPLES  2^23  > 0, else 2^23  samples per batch where the params give none. Each batch pays the shadow
    //   pass's host round trips and every level's, so a handle that renders frame after frame takes the whole frame in
    //   one batch (frt_render_params.batch_samples; 8 M / 32 M / 128 M samples per batch gave 54.3 / 49.1 / 48.0 ms
    //   headline frames, tools/ab_batch.sh). The default suits one-shot calls (render_multi): a handle's first frame
    //   allocates its level state, and the driver clears fresh device memory at ~11 GB/s, 6 s for 128 M samples
    //   (tools/rm_batch.py, profiles/r04_ab_batch.txt)
    int64_t batch_samples = (int64_t)1 << 23;
    // FRT_EYE_CAM  on  0 off  level 0 leaves eyev to camera_eyev; off: level 0 stores eyev too (A/B)
    bool eye_cam = true;
    // FRT_HEAD_KEY0  on  0 off  level 0 stores its keys for a multi-row light (shipped frame 56.4 -> 59.3 ms with the
    //   derived key, profiles/r08_ab_head_cols.txt); off: level 0 derives them there too (A/B, tests/test_head_cols.py)
    bool head_key0 = true;
    // FRT_CAM_FAST  on  0 off  level 0's camera arithmetic in its cheap exact form: a batch whose sample and pixel
    //   indices fit 32 bits divides by multiply-shift (frt_cam_index.hpp), and a camera without an aperture takes its
    //   rays' one origin from the host (DevScene::cam_origin); off: the 64-bit divisions and the origin per ray. The
    //   same bits either way (tests/test_camera_fast.py; A/B: profiles/r10_ab_camera.txt)
    bool cam_fast = true;
    // FRT_SHADE_SPLIT  on  "0" off  shading in two kernels (k_shade lists the nodes with light-point work, k_shade_lit
    //   shades them); off: one kernel for every node (A/B)
    bool shade_split = true;
    // FRT_SHADE_LAZY  on  "0" off  the ambient-only nodes' terms computed by k_combine instead of stored by k_shade
    //   (with the split and without GI); off: stored (A/B)
    bool shade_lazy = true;
    // FRT_FUSE_RESOLVE  on  "0" off  level 0 combined and resolved in one pass when a block holds whole pixels; off:
    //   the two kernels (A/B)
    bool fuse_resolve = true;
    // FRT_JIT_MAX_PAIRS  0 (none)  1..2^31-1, else 0  lowers the pair kernels' 2^31 - 1 pairs per launch (the tests
    //   split small batches this way)
    int64_t jit_max_pairs = 0;
    // FRT_JIT_MIN_PAIRS  2^18  any integer  levels with fewer (node, part) pairs skip the beam stages: each stage's
    //   launch is sized on the host from the previous one's counts, a round trip (~15 us plus the idle GPU) that costs
    //   more than walking their rays one by one; the per-ray walk of every pair gives the same counts
    int64_t jit_min_pairs = (int64_t)1 << 18;
    // FRT_JIT_SUBTILE_DEEP  on  0 off  off: levels past the camera's walk the sub-part list ray by ray (A/B)
    bool jit_subtile_deep = true;
    // FRT_JIT_SUPERTILE_DEEP  off  non-zero on  the levels that decide super-tiles first (FRT_JIT_SUPERTILE): level 0
    //   only, whose nodes are pixel-major, or (on) every level that takes the beam stages; the deeper levels' nodes are
    //   in parent order. Headline frame: level 0 only 24.13 ms, every level 23.98 ms (0.15 ms, under three spreads of
    //   0.13 ms); cornell_direct_800_4x4: 2.69 against 2.81 ms (round 11, profiles/r11_ab_supertile.txt)
    bool jit_supertile_deep = false;
    // FRT_JIT_TRACE (frame side)  on  0 off  use the scene's frt_jit_trace where it has one
    bool jit_trace = true;
    // FRT_JIT_TRACE_STATS  off  set: on  debug: the undecided share per launch (synchronises)
    bool jit_trace_stats = false;
    // FRT_JIT_TRACE_DUMP  unset  a path  with the stats: the level-0 list of undecided rays, int32 ray indices
    std::string jit_trace_dump;
    // FRT_GATHER_CHUNK  2^24  >= 1024, else 2^24  gather rays per chunk: each chunk's estimate launch ends in a tail of
    //   its slowest queries; 2^22 / 2^24 / 2^25 rays gave 29.33 / 28.97 / 28.92 s GI frames
    //   (profiles/r05_ab_gi_chunk.txt); 2^24 keeps the chunk's buffers at 3.2 GB
    int64_t gather_chunk = (int64_t)1 << 24;
    // FRT_GATHER_JIT  on  0 off  the hemisphere rays through the scene-specialised closest hit where the scene has one
    //   (1387 -> 1363 ms per cornell_gi_480x270_8x8 frame, profiles/r06_ab_gather_jit.txt; round 4's slower kernel lost
    //   there, profiles/r04_ab_gi_trace.txt); off: the generic walk (A/B)
    bool gather_jit = true;
    // FRT_GATHER_QUEUE  on  "0" off  off: the static request ranges (A/B)
    bool gather_queue = true;
    // FRT_GATHER_SORT  -1  any int  the requests in the spatial order of their points from 4096 of them; 0: gather
    //   order, 1: sorted at any count
    int gather_sort = -1;
    // FRT_SHARE_PHOTONS  on  0 off  off: every handle traces its own photon maps (A/B)
    bool share_photons = true;
    // FRT_GI_TIMING  off  set: on  diagnostics: host-side phase times of the photon pass
    bool gi_timing = false;
    // FRT_PM_CELL_DIV  3.0  1.0..16.0, else 3.0  photon grid cells per irradiance radius (A/B experiments only)
    double pm_cell_div = 3.0;
    // FRT_PM_MAX_CELLS_LOG2  0 (the engine's kMaxGridCells)  10..30, else 0  the grid's cell budget as a power of two
    //   (A/B experiments only)
    int pm_max_cells_log2 = 0;
};

inline FrameKnobs read_frame_knobs() {
    using namespace frt_knobs;
    FrameKnobs k;
    if (const char* e = raw("FRT_PRECISION")) k.precision = e;
    const long long batch = ll_or("FRT_BATCH_SAMPLES", 0);
    if (batch > 0) k.batch_samples = (int64_t)batch;
    k.eye_cam = unless_int0("FRT_EYE_CAM");
    k.head_key0 = unless_int0("FRT_HEAD_KEY0");
    k.cam_fast = unless_int0("FRT_CAM_FAST");
    k.shade_split = unless_str0("FRT_SHADE_SPLIT");
    k.shade_lazy = unless_str0("FRT_SHADE_LAZY");
    k.fuse_resolve = unless_str0("FRT_FUSE_RESOLVE");
    const long long mp = ll_or("FRT_JIT_MAX_PAIRS", 0);
    k.jit_max_pairs = mp >= 1 && mp < (1ll << 31) ? (int64_t)mp : 0;
    k.jit_min_pairs = (int64_t)ll_or("FRT_JIT_MIN_PAIRS", 1ll << 18);
    k.jit_subtile_deep = unless_int0("FRT_JIT_SUBTILE_DEEP");
    k.jit_supertile_deep = int_or("FRT_JIT_SUPERTILE_DEEP", 0) != 0;
    k.jit_trace = unless_int0("FRT_JIT_TRACE");
    k.jit_trace_stats = present("FRT_JIT_TRACE_STATS");
    if (const char* d = raw("FRT_JIT_TRACE_DUMP")) k.jit_trace_dump = d;
    const long long chunk = ll_or("FRT_GATHER_CHUNK", 0);
    if (chunk >= 1024) k.gather_chunk = (int64_t)chunk;
    k.gather_jit = unless_int0("FRT_GATHER_JIT");
    k.gather_queue = unless_str0("FRT_GATHER_QUEUE");
    k.gather_sort = int_or("FRT_GATHER_SORT", -1);
    k.share_photons = unless_int0("FRT_SHARE_PHOTONS");
    k.gi_timing = present("FRT_GI_TIMING");
    if (const char* e = raw("FRT_PM_CELL_DIV")) {
        const double v = std::atof(e);
        if (v >= 1.0 && v <= 16.0) k.pm_cell_div = v;
    }
    const int cells = int_or("FRT_PM_MAX_CELLS_LOG2", 0);
    k.pm_max_cells_log2 = cells >= 10 && cells <= 30 ? cells : 0;
    return k;
}

// frt_device_warmup's knobs (no handle exists yet): read at that function's entry
struct WarmupKnobs {
    // FRT_WARMUP_TRACE  off  set: on  each warm-up step's time to stderr
    bool trace = false;
    // FRT_WARMUP_MODE  0  any int  1: the null stream instead of a stream of its own (probes only)
    int mode = 0;
};

inline WarmupKnobs read_warmup_knobs() {
    WarmupKnobs k;
    k.trace = frt_knobs::present("FRT_WARMUP_TRACE");
    k.mode = frt_knobs::int_or("FRT_WARMUP_MODE", 0);
    return k;
}
