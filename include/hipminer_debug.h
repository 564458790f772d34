/*
 * hipminer_debug.h -- test hooks and debug exports of libhipminer.so.
 *
 * Not part of the drop-in boundary (hipminer.h): the suite and bench.py use
 * these to reach paths a small range would not take and to look inside the
 * library.  They may change with any ABI minor.
 */
#ifndef HIPMINER_DEBUG_H
#define HIPMINER_DEBUG_H

#include "hipminer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test and experiment hooks for hm_set_option (ids as they always were). */
#define HM_OPT_TABLE_DIGITS 7  /* test hook (-1..7, 0 = default 7): the final-
                                  block digits one K+W table of the chained
                                  kernel covers; the remaining high final-block
                                  digits run as epochs (one table each).  Smaller
                                  values exercise the epochs on small ranges;
                                  -1 keeps final blocks of >= 5 digits on the
                                  tiled kernel (ABI 1.5)                        */
#define HM_OPT_TABLE_ROWS_CAP 8 /* test hook (>= 0, 0 = off): a K+W table may not
                                  grow beyond this many rows, as if the device
                                  were out of memory; the chained layout then
                                  falls back to smaller tables and more epochs
                                  (the HM_ERR_NOMEM path of table growth; ABI
                                  1.6)                                          */
#define HM_OPT_TEST_MID_SYNC 9  /* test hook (0/1): the call waits on the host for
                                  each device's first queued work while still
                                  enqueuing, which hm_stats.mid_call_syncs must
                                  count (ABI 1.7)                               */
#define HM_OPT_FUSED_FLAGS 11   /* experiment hook (0..31, default 1): how the fused
                                  launch's waves get tasks -- bit 0: first task =
                                  the wave's slot (no opening burst of queue
                                  atomics; the shipped scheme); bit 1: dequeue
                                  the next task while the current one runs; bit
                                  2: no queue, wave slots strided over the task
                                  ids; bit 3: dequeue through the workgroup's
                                  LDS dispenser (ABI 1.7); bit 4: a wave's
                                  priority falls with the tasks it ran (ABI 1.8).
                                  Bits 1..4 measured and rejected   */
#define HM_OPT_FUSED_PARTS 12   /* experiment hook (1, 2, 5, 10; default 1): a
                                  tiled task of the fused launch covers 10 /
                                  parts steps of its units loop (ABI 1.7);
                                  2, 5, 10 measured and rejected                */
#define HM_OPT_QUEUE_BATCH 17   /* experiment hook (0, 4, 8, 16, 32; ABI 1.8):
                                  tasks a workgroup fetches per work-queue
                                  atomic in the per-segment kernels; 0 (default)
                                  = 4, and 16 for launches of >= 10^11 nonces */
#define HM_OPT_VERIFY_CHUNK 19  /* test hook (a multiple of 64 in [64, 2^22];
                                  0 = default 2^22; ABI 1.12): list elements
                                  per chunk and device of the list calls, so a
                                  list of a few hundred records crosses chunk
                                  boundaries (ids 16 and 18 stay retired)      */
#define HM_OPT_FIND_WINDOW 20   /* test hook (64..2^27; 0 = default 2^27; ABI
                                  1.13): nonces of a request that hm_find_many
                                  runs as its fused launch, so a test can put
                                  the window's end anywhere                    */
#define HM_OPT_VERIFY_JOBS 21   /* test hook (1..4096; 0 = default 4096; ABI
                                  1.14): jobs one hm_verify_many launch holds,
                                  so a batch of a few requests crosses launch
                                  boundaries; with HM_OPT_VERIFY_CHUNK, which
                                  that call honours as its records bound       */
#define HM_OPT_COLLECT_WINDOW 22 /* test hook (64..2^27; 0 = default 2^27; ABI
                                  1.15): a request of more nonces than this is
                                  not fused by hm_collect_many, so a test can
                                  put the fused/unfused boundary at a few
                                  hundred nonces                               */
#define HM_OPT_FIND_K_BUF 23    /* test hook (1..2^24; 0 = default min(2^24,
                                  2k + 4096); ABI 1.16): records of the device
                                  buffer hm_find_k collects into (a call uses
                                  at least its k), so a test can force the
                                  overflow path with a few hundred nonces      */

/* The embedded scan code object: *p = its first byte, returns its size.
 * bench.py hashes these bytes to match a PMC summary to the build that runs. */
size_t hm_debug_code_object(const unsigned char **p);

/* The deadline HM_OPT_DEADLINE_MS = -1 gives one request on `cus` compute
 * units, in ms (-1.0 if planning failed).  Host-only. */
double hm_debug_auto_deadline_ms(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
                                 int cus);

/* Streams (hardware queues) made so far on device i of ctx: 1 after hm_open,
 * up to HM_OPT_STREAMS once calls used them; -1 if i is out of range. */
int hm_debug_streams_made(const hm_ctx *ctx, int i);

/* Test hook of hm_cancel (ABI 1.18).  on != 0: the find-family launches of ctx
 * get a null cancel pointer (no relay wave) and the host does not test the
 * cancel flag, so a call that hm_cancel signalled (it still returns 1) runs to
 * its end: what stops a launch is the relay.  A debug export, not an option id:
 * the ids of hm_set_option end at 23.  HM_ERR_INVALID for ctx == NULL. */
int hm_debug_no_relay(hm_ctx *ctx, int on);

/* The planner's digit segments of [lo, hi] for msg: up to `cap` descriptors of
 * 13 x int64 each -- d, lo, hi, kind, W1, V, trailer, straddle, seg_cost
 * (SIMD cycles / 64 nonces), lane3, f, tch, fe (the last three chained only).
 * Returns the number of segments (may exceed cap).  Host-only. */
int hm_debug_plan(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, int force_generic,
                  int64_t *outv, int cap);

#ifdef __cplusplus
}
#endif

#endif /* HIPMINER_DEBUG_H */
