/* splat_retain.h -- RETAINED LISTS: may a frame composite from the tile lists an earlier frame left in order in memory?
 *
 * With a camera at rest and an unchanged scene every frame's binning (K1, scan), ordering (near selection or sort launches)
 * and in-compositor list sort produce what the previous frame's did.  The frame scheduler (enqueue_frame, splat_api.hip)
 * therefore launches ONE such frame with the compositor's write-back on -- the WRITER: its slot then holds records, tile
 * table and every list in the order the walks read -- and composites the frames that follow from that slot alone, for as
 * long as nothing that places a Gaussian on the target has changed.
 *
 * The decision is this pure function (no HIP call, no context, no allocation; tests/test_retain_decide.py drives it on a box
 * without a GPU).  What it is given:
 *   - the camera, as the BYTES the call received plus the slab (compared bytewise with the previous frame's and the
 *     writer's: the frame policy's 64-bit camera hash never decides that two cameras are the same one);
 *   - the context's BINNING EPOCH: a counter the library bumps wherever something K1, the scan or the ordering would read
 *     or produce has changed (scene, edit, slab, option, target, key buffers, layouts dropped, a count-only pass);
 *   - the frame policy's still-frame count, the frame overlap, the binning path, and the writer's status as the host sees it.
 * Not part of the reference's operator surface (include/splat_hip.h is): a diagnostic interface, versioned by struct size. */
#ifndef SPLAT_RETAIN_H
#define SPLAT_RETAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_RETAIN_CAM_WORDS 48        /* splat_camera (44 words) + the slab's two tile rows, zero-padded */

#define SPLAT_RETAIN_BIN 0               /* an ordinary frame: binned, ordered, composited */
#define SPLAT_RETAIN_WRITER 1            /* an ordinary frame whose compositor writes its sorted short lists back (the writer) */
#define SPLAT_RETAIN_RETAIN 2            /* the compositor alone, on the writer's slot */

typedef struct splat_retain_state {      /* carried from frame to frame; all zeros = nothing known */
    uint32_t have_cam;                   /* last_cam holds the previous frame's camera */
    uint32_t same_run;                   /* frames in a row whose camera bytes and epoch equal the previous frame's */
    uint32_t writer;                     /* 0 none, 1 launched (its status decides at the next frame), 2 established: a set is retained */
    uint32_t pad_;
    uint64_t epoch;                      /* the previous frame's binning epoch */
    uint32_t last_cam[SPLAT_RETAIN_CAM_WORDS];
} splat_retain_state;

typedef struct splat_retain_input {
    uint32_t cam[SPLAT_RETAIN_CAM_WORDS];
    uint64_t epoch;
    uint32_t still_frames;               /* splat_policy_state::still_frames after this frame's policy decision */
    int32_t enabled;                     /* SPLAT_OPT_RETAIN_LISTS */
    int32_t overlap;                     /* splat_set_frame_overlap: 2 = a second compositor lane -- no retention */
    int32_t one_pass;                    /* one-pass binning; two-pass frames are never retained */
    /* the writer's status (state.writer == 1), as harvested or peeked */
    uint32_t writer_arrived, writer_overflow, writer_redone;
    uint32_t pad_;
} splat_retain_input;

typedef struct splat_retain_decision {
    int32_t action;                      /* SPLAT_RETAIN_BIN / _WRITER / _RETAIN */
    int32_t ended;                       /* 1: an established set ended with this frame */
    int32_t wait_for_writer;             /* 1: everything says "retain" but the writer's status has not arrived: the scheduler may wait
                                            for that frame and ask again with its status (the decision as it stands does not retain) */
    int32_t pad_;
    splat_retain_state next;
} splat_retain_decision;

/* 0, or -1 for a NULL argument.  Pure: the same arguments give the same decision. */
int splat_retain_decide(const splat_retain_state* state, const splat_retain_input* in, splat_retain_decision* out);
/* sizeof the three structs above, in declaration order, as the LIBRARY was built */
void splat_retain_struct_sizes(uint64_t sizes[3]);

#ifdef __cplusplus
}
#endif
#endif
