// TEST HARNESS (not product code): the seeding functions of centerpose_amd/csrc/track_common.h compiled for the host with
// g++ (tests/test_track_seed_cpu.py), next to the frame stages of tests/native/track_host.cpp so that a seeded list can be
// stepped like any other.  The product runs the same functions inside track.hip's track_seed_kernel.
#include "../../centerpose_amd/csrc/track_common.h"

#include <vector>

extern "C" {
int cp_seed_host_stride(void) { return CP_SEED_STRIDE; }
int cp_seed_host_track_stride(void) { return CP_TRACK_STRIDE; }
int cp_seed_host_params_bytes(void) { return (int)sizeof(TrackParams); }

// what track_seed_kernel does for one video: seeds [ns][CP_SEED_STRIDE] -> tracks [cap][CP_TRACK_STRIDE], recs [cap][9][5]
// (all cap rows); returns the length of the list, *id_count = last id given out, *dropped = seeds beyond cap
int cp_seed_host_seed(const TrackParams* P, const double* vm, const double* seeds, int ns, int gt, int hm_plane, int hp_plane0,
                      double* tracks, double* recs, int* id_count, int* dropped) {
    std::vector<int> accepted(P->cap > 0 ? P->cap : 1);
    const int n = trk_seed_walk(*P, seeds, ns, accepted.data(), id_count, dropped);
    for (int e = 0; e < P->cap; ++e) {
        double* rec = recs + (size_t)e * 45;
        if (e < n)
            trk_seed_stage(*P, vm, seeds + (size_t)accepted[e] * CP_SEED_STRIDE, e + 1, gt, hm_plane, hp_plane0,
                           tracks + (size_t)e * CP_TRACK_STRIDE, rec);
        else
            for (int i = 0; i < 9; ++i) rec[5 * i] = -1.0;
    }
    return n;
}

// stages 1-3 of one frame of one video, as cp_track_host_update of track_host.cpp (greedy association)
int cp_seed_host_update(const TrackParams* P, const double* vm, const double* post, int count, const double* prev, int np,
                        int* id_count, double* next, float* pts, float* scale) {
    const int c1 = count > 0 ? count : 1;
    std::vector<double> dets((size_t)c1 * CP_TRACK_STRIDE);
    std::vector<int> use(c1), idx(c1), plan((size_t)3 * (P->cap > 0 ? P->cap : 1));
    std::vector<unsigned char> taken(np > 0 ? np : 1);
    int any = 0, dropped = 0;
    for (int k = 0; k < count; ++k) {
        use[k] = trk_prepare_det(*P, vm, post + (size_t)k * 120, nullptr, dets.data() + (size_t)k * CP_TRACK_STRIDE);
        any |= use[k];
    }
    if (!any)
        for (int k = 0; k < count; ++k) use[k] = 1;
    const int n = trk_associate(*P, dets.data(), use.data(), count, prev, np, plan.data(), id_count, idx.data(), taken.data(),
                                &dropped);
    for (int t = 0; t < n; ++t)
        trk_materialise(plan.data() + 3 * t, dets.data(), prev, next + (size_t)t * CP_TRACK_STRIDE, 0, CP_TRACK_STRIDE);
    for (int t = 0; t < n; ++t)
        trk_track_stage(*P, next + (size_t)t * CP_TRACK_STRIDE, prev, pts + (size_t)t * 16, scale + (size_t)t * 3);
    return n;
}

}  // extern "C"
