// splat_retain.cpp -- retained lists: the decision (include/splat_retain.h).  Plain host C++: no HIP header, no context,
// nothing allocated; enqueue_frame (splat_api.hip) calls it once per frame, behind the frame policy.
#include <algorithm>
#include <cstring>

#include "../../include/splat_policy.h"
#include "../../include/splat_retain.h"

extern "C" {

void splat_retain_struct_sizes(uint64_t sizes[3]) {
    if (!sizes) return;
    sizes[0] = sizeof(splat_retain_state); sizes[1] = sizeof(splat_retain_input); sizes[2] = sizeof(splat_retain_decision);
}

int splat_retain_decide(const splat_retain_state* sp, const splat_retain_input* ip, splat_retain_decision* out) {
    if (!sp || !ip || !out) return -1;
    const splat_retain_input& in = *ip;
    splat_retain_decision d;
    std::memset(&d, 0, sizeof d);
    d.next = *sp;
    splat_retain_state& st = d.next;
    // the same camera, byte for byte, under the same epoch as the frame before?
    const bool same = sp->have_cam != 0u && sp->epoch == in.epoch && std::memcmp(sp->last_cam, in.cam, sizeof in.cam) == 0;
    st.same_run = same ? std::min(sp->same_run + 1u, 1000000u) : 0u;
    st.have_cam = 1u; st.epoch = in.epoch;
    std::memcpy(st.last_cam, in.cam, sizeof in.cam);
    // (two compositor lanes could repair the same tile's storage at once; a two-pass frame's lists are exactly sized and its
    // counters must be zero between frames: neither is retained)
    const bool allowed = in.enabled != 0 && in.overlap < 2 && in.one_pass != 0;
    if (!same || !allowed) { d.ended = sp->writer == 2u ? 1 : 0; st.writer = 0u; }
    d.action = SPLAT_RETAIN_BIN;
    if (allowed && same) {
        if (st.writer == 1u) {
            // the frame before this one was launched as the writer: a complete frame binned once establishes the set
            const bool clean = in.writer_arrived != 0u && in.writer_overflow == 0u && in.writer_redone == 0u;
            d.wait_for_writer = in.writer_arrived == 0u ? 1 : 0;
            st.writer = clean ? 2u : 0u;
        }
        if (st.writer == 2u) d.action = SPLAT_RETAIN_RETAIN;
        // at rest for as long as the start hints ask (every frame in flight then comes from this camera), by both counts
        else if (std::min(st.same_run, in.still_frames) >= (uint32_t)SPLAT_POLICY_STILL_FRAMES) { d.action = SPLAT_RETAIN_WRITER; st.writer = 1u; }
    }
    *out = d;
    return 0;
}

}  // extern "C"
