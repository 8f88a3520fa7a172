// frt-mi355x shadow pass pieces shared by the engine's k_shadow and the
// scene-specialised shadow kernels generated at upload (frt_jit.cpp): the
// per-(path node, light sample) lane setup of is_shadowed (renderer.c:74-93)
// and the segmented reduction of unshadowed counts.
#pragma once

#include "frt_traverse.hpp"

namespace frt {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// area-light cache row for (path node, light, draw): the reference draws
// rand() % cache_len twice per (hit, light) (light.c:196, renderer.c:915);
// with a single-row cache both are row 0, as in the reference
__device__ __forceinline__ int light_row_n(int rows, uint64_t seed, uint64_t key, int light, int draw) {
    if (rows <= 1) return 0;
    uint64_t h = mix64(seed ^ mix64(key * 0x9e3779b97f4a7c15ULL + (uint64_t)(light * 2 + draw + 1)));
    return (int)(h % (uint64_t)rows);
}

__device__ __forceinline__ int light_row(const frt_light& L, uint64_t seed, uint64_t key, int light, int draw) {
    return light_row_n(L.rows, seed, key, light, draw);
}

// Ray queues of the levels are segmented: a block appends to segment
// blockIdx % kQueueSegs through that segment's own counter (one per 256-byte
// line), because device-scope atomics on one address serialise (~12 ns each:
// tools/microbench/atomics.hip). Segment j of a level's queue holds entries
// [qprefix[j], qprefix[j+1]) of the level at j * qsegcap + (i - qprefix[j]).
constexpr int kQueueSegs = 64;
constexpr int kCounterLine = 32;  // 8-byte words per counter line (256 bytes)

struct Batch {
    int64_t sample_begin;  // first global sample index of the batch
    int64_t pixel_begin;   // first pixel (in render order) of the batch
    int64_t num_samples;
    int64_t row_begin, row_stride;
    uint64_t seed;
    int32_t spp, level;
    int32_t remaining;     // path_length - level
    int32_t stats;         // the frame collects statistics (frt_frame_stats): the diagnostic counters are counted
    const int64_t* qprefix;  // this level's queue segments (kQueueSegs + 1 prefix counts); null: contiguous
    int64_t qsegcap;         // entries per segment of this level's queue
    int64_t next_segcap;     // entries per segment of the next level's queue
    const uint32_t* qperm;   // the level's entries in parent order: entry i at storage slot qperm[i]; null: the segments
    // level 0's index math in 32 bits (frt_camera.hpp camera_sample), decided on the host where the batch is filled
    // (frt_cam_index.hpp cam_index_fits32, FRT_CAM_FAST): the multiply-shift constants of / spp and / hsize
    uint32_t cam_fast;       // 0: the 64-bit divisions
    uint32_t spp_magic, spp_shift, hs_magic, hs_shift;
};

// storage slot of entry i of the level's queue
__device__ __forceinline__ int64_t queue_slot(const Batch& B, int64_t i) {
    if (B.qperm != nullptr) return B.qperm[i];
    if (B.qprefix == nullptr) return i;
    int lo = 0, hi = kQueueSegs;  // the last segment j with qprefix[j] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (B.qprefix[mid] <= i) lo = mid;
        else hi = mid;
    }
    return (int64_t)lo * B.qsegcap + (i - B.qprefix[lo]);
}

// key of sample s of a batch's level 0 (frt_camera.hpp: the key camera_ray gives the sample's ray)
__device__ __forceinline__ uint64_t camera_key(const DevScene& S, const Batch& B, int64_t s);

// What the shadow pass reads of a level's path nodes, as columns of the level's capacity (the pass re-reads it from
// 100 lanes; apart from the path-node columns, its HBM traffic stays at about one line per node): over_point as three
// columns of doubles (coordinate a of node i at op[a * cap + i]: a wave's k_prepare stores are three 512-byte runs)
// and the nodes' keys where they cannot be derived. A level 0 whose rays are camera_ray's stores no keys (key ==
// nullptr): node i's is camera_key(S, B, node0 + i). Whether a node has a hit to shade is the material word of its
// path-node record (NodeCols core word 0, -1 for a miss), which k_prepare writes for every node: mat is that column.
struct HeadCols {
    double* op = nullptr;
    uint64_t* key = nullptr;
    const uint64_t* mat = nullptr;
    int64_t cap = 0;
    int64_t node0 = 0;  // the level's index of the view's node 0 (a node range of the level: at())

    // the nodes from off on (the same columns: the stride stays the level's capacity)
    __host__ __device__ HeadCols at(int64_t off) const {
        HeadCols v = *this;
        v.op += off;
        if (v.key != nullptr) v.key += off;
        v.mat += off;
        v.node0 += off;
        return v;
    }
    __device__ __forceinline__ bool hit(int64_t i) const { return (int32_t)(uint32_t)mat[i] >= 0; }
    __device__ __forceinline__ void over_point(int64_t i, double* o) const {
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = op[a * cap + i];
    }
};

__device__ __forceinline__ uint64_t head_key(const DevScene& S, const Batch& B, const HeadCols& H, int64_t i) {
    return H.key != nullptr ? H.key[i] : camera_key(S, B, H.node0 + i);
}

// one lane per (path node, light sample j); lanes of a node are consecutive
struct ShadowLane {
    Ray r;
    double distance;
    int64_t node;
    int light;
    bool valid;  // tid < n * samples_per_node
    bool live;   // the node has a hit to shade
};

__device__ __forceinline__ void shadow_lane(const DevScene& S, const Batch& B, const HeadCols& shead,
                                            int64_t n, const int32_t* __restrict__ j_light,
                                            const int32_t* __restrict__ j_point, int32_t samples_per_node,
                                            int64_t tid, ShadowLane& L) {
    L.valid = tid >= 0 && tid < n * samples_per_node;
    L.node = 0;
    L.light = 0;
    L.live = false;
    L.r = Ray{{0, 0, 0}, {0, 0, 1}};
    L.distance = 0.0;
    if (L.valid) {
        L.node = tid / samples_per_node;
        const int j = (int)(tid % samples_per_node);
        L.light = j_light[j];
        const int pt = j_point[j];
        if (shead.hit(L.node)) {
            L.live = true;
            const frt_light& lt = S.lights[L.light];
            const int row = lt.rows <= 1 ? 0 : light_row(lt, B.seed, head_key(S, B, shead, L.node), L.light, 0);
            const double* lp = S.light_points + lt.points + 3 * ((int64_t)row * lt.num_samples + pt);
            // is_shadowed (renderer.c:74-93)
            double op[3];
            shead.over_point(L.node, op);
            double v[3] = {lp[0] - op[0], lp[1] - op[1], lp[2] - op[2]};
            L.distance = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            L.r.o[0] = op[0];
            L.r.o[1] = op[1];
            L.r.o[2] = op[2];
            normalize3(v, L.r.d);
        }
    }
}

// segmented wave reduction: lanes with the same (node, light) are contiguous;
// one integer atomic per segment
__device__ __forceinline__ void shadow_count(const DevScene& S, const ShadowLane& L, bool lit, int32_t* counts) {
    const int lane = threadIdx.x & 63;
    const int64_t key = L.valid ? L.node * S.num_lights + L.light : -1 - (int64_t)lane;
    const int64_t prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long lits = __ballot(lit);
    if (L.valid && head) {
        const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
        const int next = above ? __ffsll((long long)above) - 1 : 64;
        const unsigned long long seg = (next >= 64 ? ~0ull : ((1ull << next) - 1)) & ~((1ull << lane) - 1);
        const int c = __popcll(lits & seg);
        if (c) atomicAdd(counts + key, c);
    }
}

}  // namespace frt
