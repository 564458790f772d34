/*
 * hipminer.h -- C ABI of the MI355X (gfx950) miner backend.
 *
 * Drop-in boundary for ONE hot path of alexsun705/distributed_bitcoinMiner:
 * the miner's min-hash scan.  Reference interfaces replaced (paths relative to
 * the reference root, cmu440/ = p1/src/github.com/cmu440/):
 *
 *   hm_hash  replaces  bitcoin.Hash(msg string, nonce uint64) uint64
 *                      cmu440/bitcoin/hash.go:13-17
 *   hm_scan  replaces  the scan loop of evalRoutine,
 *                      cmu440/bitcoin/miner/miner.go:46-59
 *                      (result = maxUint; index = 0; for i := lower; i < upper;
 *                       i++ { hash := bitcoin.Hash(data, i); if hash < result ...})
 *                      fed by bitcoin.Message{Data, Lower, Upper}
 *                      (cmu440/bitcoin/message.go:18-23) and producing the
 *                      values of bitcoin.NewResult(hash, nonce) (:38-44).
 *
 * hm_find (ABI 1.10) adds the proof-of-work form of that loop, which the
 * reference does not have: the LOWEST nonce whose hash is below a target,
 * found without scanning the rest of the range.  hm_collect (ABI 1.11) adds
 * its share-collection form: EVERY nonce whose hash is below a target, and
 * their exact count.  The list calls of ABI 1.12 are the receiving side of
 * that exchange, which the reference's server lacks (server.go:273 believes
 * the hash it is sent): the hash at every nonce of a list, and which
 * (hash, nonce) records of a list are wrong or not below a target.
 * hm_scan_k (ABI 1.19) is the ranking form: the k lowest (hash, nonce) pairs
 * of a range, the reference's minimum being k = 1.
 *
 * The cgo binding a maintainer adds to the Go miner is in INTEGRATION.md.
 *
 * Semantics (bit-exact with the reference):
 *   - bytes hashed per nonce: msg[0..len) ‖ 0x20 ‖ decimal(nonce)   (hash.go:15)
 *   - key: first 8 bytes of SHA-256, big-endian                      (hash.go:16)
 *   - hm_scan: lexicographic min of (key, nonce) over the INCLUSIVE range
 *     [lo, hi], seeded with (UINT64_MAX, 0).  This equals the reference's
 *     ascending strict-< loop, ties to the lowest nonce.  lo > hi gives
 *     (UINT64_MAX, 0).  hi may be UINT64_MAX: the reference miner's
 *     `upper := Upper+1` wrap (miner.go:52) is NOT applied here; callers that
 *     mirror evalRoutine apply it (see distributed_bitcoinminer_amd/miner.py).
 *
 * Ownership: msg is borrowed for the call only (never retained), so a cgo
 * caller may pass Go memory.  `out` is written only when the call returns
 * HM_OK.  The context owns its device buffers and streams.
 *
 * Threading: calls on one context are serialised by an internal mutex; every
 * call re-binds its device (hipSetDevice), so Go may call from any OS thread.
 * hm_close must not race other calls on the same context (the caller owns
 * the context's lifetime, as with any C handle).  hm_cancel (ABI 1.18) is the
 * one call that does not take that mutex: it may run while another thread is
 * inside a call on the context.
 *
 * Errors: 0 = HM_OK; negative codes below; hm_strerror() describes them.
 * Nothing aborts the process, and a failed GPU scan is reported, never
 * silently replaced.  With HM_OPT_DEADLINE_MS a scan that the GPU does not
 * finish in time returns HM_ERR_TIMEOUT instead of blocking (ABI 1.8).  hm_scan_cpu (ABI 1.7) is the host scan a caller may
 * choose when hm_open or hm_scan fails, so that a Result is still written
 * (SURVEY §8(b)); the GPU entry points never call it.
 */
#ifndef HIPMINER_H
#define HIPMINER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 16 bytes: the (hash, nonce) candidate; also the RCCL all-gather element. */
typedef struct hm_result {
    uint64_t hash;
    uint64_t nonce;
} hm_result;

typedef struct hm_ctx hm_ctx;

/* Timing and work accounting of the most recent hm_scan on a context. */
typedef struct hm_stats {
    double wall_ms;          /* host wall time of the hm_scan call              */
    double kernel_ms;        /* time during which some scan kernel ran: union of
                                the launches' HIP-event intervals, summed over
                                devices                                          */
    double dom_kernel_ms;    /* summed duration of the dominant scan kernel's
                                launches (dominant = most nonces; one kernel
                                instantiation may serve several segments)       */
    uint64_t nonces;         /* nonces covered by the call                       */
    uint64_t dom_nonces;     /* nonces covered by the dominant kernel            */
    uint64_t dom_compressions; /* SHA-256 compressions per nonce after the host
                                  midstate in the dominant kernel's segments (C
                                  of SURVEY §8d; algorithmic, before hoisting)  */
    int32_t launches;        /* scan-kernel launches issued                      */
    int32_t dom_kind;        /* HM_KIND_* of the dominant kernel                 */
    int32_t ndev;            /* devices used                                      */
    int32_t dom_grid;        /* workgroups of the dominant kernel's largest launch */
    int32_t dom_launches;    /* launches of the dominant kernel                  */
    int32_t merge;           /* HM_MERGE_*: how the per-device 16-B results were
                                merged (ABI 1.4; was reserved)                   */
    char dom_kernel[64];     /* its name as rocprofv3 lists it (without args)   */
    double dom_compressions_eff; /* SHA-256 compressions per nonce the dominant
                                  kernel executes (ABI 1.4): dom_compressions
                                  minus the work hoisted out of the per-nonce
                                  loop.  Tiled: 1 (+1 with a constant trailer
                                  block); chained: 1 + 1/tch, the per-lane block
                                  0 amortised over tch loop values (f <= 4
                                  final-block digits: tch = min(10^f, 1000);
                                  f >= 5: tch = min(10^fe, 100), fe the table
                                  digits) (counted exactly per launch since ABI
                                  1.5: one block-0 compression per task and
                                  lane, guided-split pieces included); generic:
                                  dom_compressions.  Mean over the dominant
                                  kernel's nonces (one instantiation may serve
                                  several segments). */
    double enqueue_ms;       /* host time the call spent enqueuing GPU work on
                                its devices (planning, K+W table allocation,
                                launches) before waiting for results, summed
                                over its chunks of <= 64 requests (ABI 1.6)     */
    int32_t mid_call_syncs;  /* host waits on GPU work issued while the call was
                                still enqueuing work for some device (ABI 1.6;
                                0: every device's work is queued before the
                                host waits on any, so devices overlap)          */
    int32_t table_grows;     /* chained K+W tables enlarged by the call; an old
                                table may still be read by queued work, so it
                                is kept (< 1/9 of the new one) until
                                hm_close, as hipFree would wait for the whole
                                device (1.7 freed it at the end of the call):
                                growth never waits on the device mid-enqueue
                                (ABI 1.6)                                       */
    double deadline_ms;      /* the deadline the call ran under (ABI 1.8;
                                HM_OPT_DEADLINE_MS; 0 = none)                    */
} hm_stats;

/* sizeof(hm_stats) by ABI version.  The struct only grows at its end. */
#define HM_STATS_SIZE_1_0 136 /* ABI 1.0 .. 1.3                                 */
#define HM_STATS_SIZE_1_4 144 /* ABI 1.4, 1.5: + dom_compressions_eff          */
#define HM_STATS_SIZE_1_6 160 /* ABI 1.6, 1.7: + enqueue_ms, mid_call_syncs,
                                 table_grows                                     */
#define HM_STATS_SIZE_1_8 168 /* ABI 1.8+: + deadline_ms                         */

#define HM_MERGE_NONE 0 /* one device: its result is read back directly      */
#define HM_MERGE_HOST 1 /* several devices: 16-B results merged on the host  */
#define HM_MERGE_RCCL 2 /* RCCL ncclAllGather of the 16-B results on the
                           devices, then a device-side lexicographic fold
                           (HM_OPT_MERGE_RCCL; any device count, incl. 1)    */

#define HM_OK 0
#define HM_ERR_INVALID (-1)   /* bad argument                                   */
#define HM_ERR_NO_DEVICE (-2) /* no usable HIP device / runtime                  */
#define HM_ERR_HIP (-3)       /* a HIP runtime call failed                       */
#define HM_ERR_NOMEM (-4)     /* device or host allocation failed                */
#define HM_ERR_RCCL (-5)      /* an RCCL call failed                              */
#define HM_ERR_INTERNAL (-6)  /* planner invariant violated                      */
#define HM_ERR_TIMEOUT (-7)   /* ABI 1.8: the call passed its HM_OPT_DEADLINE_MS
                                 deadline before the GPU finished.  The context
                                 is ABANDONED: its queued work may still run, so
                                 every later call on it returns HM_ERR_TIMEOUT
                                 without touching a device, and hm_close frees
                                 only host memory (device buffers and streams
                                 are left to the process exit).  `out` is not
                                 written: the caller answers from hm_scan_cpu or
                                 a new context.                                  */
#define HM_ERR_CANCELLED (-8) /* ABI 1.18: hm_cancel stopped the call.  Nothing is
                                 written, every launch the call queued has ended
                                 and the context is fully usable                  */

#define HM_KIND_NONE 0
#define HM_KIND_GENERIC 1  /* one nonce per lane, generic tail builder          */
#define HM_KIND_TILED 2    /* tile-planned final block (lane + loop digits)      */
#define HM_KIND_CHAINED 3  /* two-block tail: per-lane block 0, table-driven final block */
#define HM_KIND_FUSED 4    /* every segment of a small request in one launch, each
                              with its own layout's task body (ABI 1.7)          */

/* Options for hm_set_option (test and experiment hooks: hipminer_debug.h).
 * Ids 16 and 18 are retired and never reused.  ABI 1.9: hm_set_option
 * returns HM_ERR_INVALID for a retired id at any value and changes nothing;
 * the context stays usable.  A caller that set one may drop the call. */
#define HM_OPT_FORCE_GENERIC 1 /* 1: route every segment to the generic kernel  */
#define HM_OPT_MERGE_RCCL 2    /* 1: merge the per-device candidates with one RCCL
                                  all-gather (also with one device: a 1-rank
                                  communicator); needs distinct device ordinals:
                                  hm_set_option returns HM_ERR_INVALID for a
                                  context that names a device twice (ABI 1.5)  */
#define HM_OPT_GRID_PER_CU 3   /* workgroups per CU for scan launches (0 = auto) */
#define HM_OPT_STREAMS 4       /* HIP streams per device for segment launches
                                  (1..4, default 4): the dominant kernel's
                                  segments on a high-priority stream, the
                                  others on low-priority streams that fill
                                  its last launch's tail; 1 = strictly serial.
                                  Since ABI 1.8 hm_open makes stream 0 only and
                                  a call makes streams 1.. when it first
                                  enqueues onto them: every HIP stream holds a
                                  hardware queue until the process exits, so a
                                  process sharing its GPU sets 1 or 2        */
#define HM_OPT_FUSED 10         /* 1 (default): a request (per device shard) of at
                                  most 2^27 nonces whose segments all fit the
                                  fused launch runs as ONE planner + ONE scan
                                  launch (HM_KIND_FUSED); 0: one launch per
                                  digit segment (ABI 1.7)                       */
#define HM_OPT_DEADLINE_MS 13   /* ABI 1.8 (SURVEY §8(b) liveness): 0 (default) =
                                  a call blocks until its GPU work is done; > 0 =
                                  a call returns HM_ERR_TIMEOUT (and abandons the
                                  context) once this many ms have passed since it
                                  began; -1 = auto: 2 s + 8 x the call's modelled
                                  kernel time (the layouts' measured cost, the
                                  model hm_partition balances with).  The host
                                  then polls the GPU instead of blocking on it.
                                  A miner whose LSP thread keeps heartbeating
                                  would otherwise hold its chunk forever: the
                                  server reassigns only dropped miners
                                  (server.go:326-376)                           */
#define HM_OPT_FUSED_TAIL 14    /* 1, 2, 5 or 10 (default 2; ABI 1.8): the tasks
                                  of a fused launch's last, partial wave-round
                                  (tasks mod waves; the cheapest layouts, queued
                                  last) run as up to this many pieces each --
                                  as many as still fit one round of the grid --
                                  so the launch does not end on a round of
                                  whole tasks with most waves idle; 1 = no
                                  split                                        */
#define HM_OPT_TAIL_FUSED 15    /* 1 (default; ABI 1.8): the segments of a large
                                  request that its dominant kernel does not run
                                  (bradfitz [0, 2^32): d <= 8) go into ONE fused
                                  launch on a low-priority stream, in the
                                  dominant launch's tail, when they fit one; 0:
                                  one launch per segment on the tail streams */
/* bitcoin.Hash (hash.go:13-17) evaluated on the host.  Not the hot path: used
 * to verify single results and for planning; needs no GPU. */
uint64_t hm_hash(const uint8_t *msg, size_t len, uint64_t nonce);

/* Open a context on `ndev` HIP devices (`devices` lists ordinals); ndev == 0
 * uses every visible device.  Returns HM_ERR_NO_DEVICE without a GPU. */
int hm_open(const int *devices, int ndev, hm_ctx **out);

/* Min-hash scan of the inclusive range [lo, hi] (see semantics above).  With
 * several devices the range is sharded contiguously and the per-device 16-B
 * candidates are merged (RCCL all-gather when HM_OPT_MERGE_RCCL is set); the
 * shards are those of hm_partition (cost-weighted). */
int hm_scan(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
            hm_result *out);

/* One request of a batch: the same meaning as hm_scan's arguments. */
typedef struct hm_request {
    const uint8_t *msg; /* borrowed for the call; may be NULL when len == 0 */
    size_t len;
    uint64_t lo, hi;    /* inclusive */
} hm_request;

/* Batch form of hm_scan: outs[i] = hm_scan(reqs[i]) for i < n.  All requests'
 * GPU work is enqueued before one host synchronisation (SURVEY §8(f) rank 4:
 * the server's FIFO (cmu440/bitcoin/server/server.go:211-219, 318-324) hands a
 * miner one small chunk at a time; a miner or a future GPU-side server can
 * batch them here).  outs is written only when the call returns HM_OK. */
int hm_scan_many(hm_ctx *ctx, const hm_request *reqs, int n, hm_result *outs);

/* Checked scan: hm_scan's result plus a coverage checksum computed on the GPU
 * by the checked variants of the same kernels (same planner, tiles, lane and
 * loop layout, guided task split and multi-device shards):
 *   *sum   = sum over n in [lo, hi] of Hash(msg, n), mod 2^64
 *   *count = number of nonces hashed (must be hi - lo + 1, mod 2^64)
 * A nonce skipped, hashed twice or hashed with wrong bytes changes the pair,
 * so it checks coverage at sizes no CPU can rescan; the sums of disjoint
 * sub-ranges add up to the sum of their union.  A verification entry point,
 * not the hot path: it runs slower than hm_scan. */
int hm_scan_checked(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
                    hm_result *out, uint64_t *sum, uint64_t *count);

/* Split the inclusive range [lo, hi] into n contiguous, ascending shards of
 * near-equal modelled GPU cost for msg (digit segments whose kernels cost more
 * per nonce get fewer nonces).  bounds[2i], bounds[2i+1] = shard
 * i's inclusive [lo, hi]; an empty shard is written as [1, 0].  The shards
 * cover [lo, hi] exactly, so per-shard hm_scan results merged by (hash, nonce)
 * minimum equal hm_scan over [lo, hi].  Host-only; needs no GPU.  This is how
 * hm_scan shards one request across a multi-device context, and what a
 * process-per-GPU caller (torch.distributed ranks, one Go miner per GPU) uses
 * to cut its range. */
int hm_partition(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, int n,
                 uint64_t *bounds);

/* Stats of the last successful hm_scan / hm_scan_many on ctx: the FIRST
 * HM_STATS_SIZE_1_4 BYTES ONLY (through dom_compressions_eff), the size the
 * ABI 1.4/1.5 headers promised.  Frozen since ABI 1.7, so a binary built
 * against any header from 1.4 on never gets more bytes than its struct
 * holds (ABI 1.6 wrote 160 bytes here, past a 1.5 caller's struct).  The
 * fields after dom_compressions_eff come only from hm_scan_stats_sized.
 * A caller built against the 1.6 header that reads enqueue_ms,
 * mid_call_syncs or table_grows MUST switch to hm_scan_stats_sized (pass
 * sizeof(hm_stats)): through this export those fields are no longer
 * written and hold whatever the caller's struct held. */
int hm_scan_stats(const hm_ctx *ctx, hm_stats *out);

/* hm_scan_stats writing at most `size` bytes (pass sizeof(hm_stats) as the
 * caller compiled it; >= HM_STATS_SIZE_1_0): the prefix of the current
 * layout that fits.  ABI 1.5.  The call to use for every field. */
int hm_scan_stats_sized(const hm_ctx *ctx, hm_stats *out, size_t size);

/* The same scan as hm_scan -- lexicographic min of (Hash(msg, n), n) over
 * the INCLUSIVE [lo, hi], seeded (UINT64_MAX, 0), bit-identical -- on the
 * host's cores, without a GPU (ABI 1.7; SURVEY §8(b)'s liveness path).
 * `threads` <= 0 uses one thread per CPU this process may run on (its
 * affinity mask, at most 1024); the range is split into that many
 * contiguous chunks (ranges below 4096 nonces per thread use fewer).
 * x86 SHA extensions when the CPU has them (HM_CPU_NO_SHA=1 forces portable
 * C).  Orders of magnitude slower than hm_scan: for callers whose GPU is
 * missing or failed (hm_miner, the Go gpuminer), so a Result is still
 * written; never called by the GPU entry points.  `out` is written only on
 * HM_OK. */
int hm_scan_cpu(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, int threads,
                hm_result *out);

/* ABI 1.10: the proof-of-work question.  The result of
 *   for n = lo .. hi (inclusive, ascending): if Hash(msg, n) < target: return (Hash, n)
 * *found = 1 and *out = (Hash(msg, n), n) for the LOWEST such n; otherwise
 * *found = 0 and *out = (UINT64_MAX, 0).  target = 0 and lo > hi never hit.
 * hi may be UINT64_MAX.  Strict '<', as in the reference's comparisons
 * (miner.go:56, server.go:273).
 *
 * The call stops early and stays exact: the kernels share one stop word per
 * device (the lowest qualifying nonce published so far), waves skip every
 * task above it, and the host enqueues launches in ascending order, at most
 * four in flight, and stops once a hit is known and everything not yet
 * issued lies above it (DESIGN.md "First below target").  Over [0, 2^64-1]
 * it returns as soon as the first hit is confirmed.
 *
 * Arguments are validated as hm_scan validates them; `out` and `found` are
 * written only on HM_OK.  An abandoned context returns HM_ERR_TIMEOUT.
 * HM_OPT_DEADLINE_MS applies (auto models the whole range: an upper bound),
 * HM_OPT_FORCE_GENERIC and HM_OPT_GRID_PER_CU are honoured; the stream,
 * fused and RCCL options do not apply: find uses stream 0, one launch per
 * segment piece, and a host merge (the lowest nonce wins).  hm_find does not
 * change what hm_scan_stats reports. */
int hm_find(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
            uint64_t target, hm_result *out, int *found);

/* The same answer as hm_find on the host's cores, no GPU (as hm_scan_cpu is
 * to hm_scan; `threads` as there).  Threads take ascending windows of the
 * range from a shared counter and stop at windows above the lowest hit. */
int hm_find_cpu(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, uint64_t target,
                int threads, hm_result *out, int *found);

/* Work accounting of the most recent successful hm_find on a context.  The
 * struct only grows at its end. */
typedef struct hm_find_stats {
    double wall_ms;           /* host wall time of the call                      */
    double kernel_ms;         /* summed HIP-event time of its find launches      */
    uint64_t nonces_enqueued; /* nonces covered by the launches actually issued.
                                 A chained launch of one epoch out of E over a
                                 span of tiles counts span / E (the last epoch
                                 the remainder too): the epochs' even share, as
                                 hm_stats counts it, not the exact nonces of
                                 that epoch inside [lo, hi]                      */
    uint64_t tasks_total;     /* tasks of those launches (a task: one wave's
                                 64 lanes x a run of loop values; generic: one
                                 grid-stride step of a wave, 64 nonces)          */
    uint64_t tasks_run;       /* tasks whose hash loop ran (the others were
                                 skipped above a published hit)                  */
    int32_t launches;         /* find-kernel launches issued                     */
    int32_t ndev;             /* devices of the context                          */
    int32_t found;            /* the call's *found                               */
    int32_t reserved;
} hm_find_stats;
#define HM_FIND_STATS_SIZE_1_10 56 /* ABI 1.10 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_FIND_STATS_SIZE_1_10) of the last successful find's stats;
 * HM_ERR_INVALID before the first one. */
int hm_find_stats_sized(const hm_ctx *ctx, hm_find_stats *out, size_t size);

/* ABI 1.13: a batch of finds.  outs[i], found[i] = what hm_find(reqs[i])
 * returns, for i < n, bit for bit: the LOWEST qualifying nonce under strict
 * '<', (UINT64_MAX, 0) with found = 0 otherwise; target = 0 and lo > hi never
 * hit; hi may be UINT64_MAX, and nonce UINT64_MAX can be an answer.
 *
 * At ordinary targets the first hit lies a few million nonces in, and hm_find
 * is bound by its launches and host round trips, not by hashing.  Here each
 * request's WINDOW -- its first 2^27 nonces, [lo, min(hi, lo + 2^27 - 1)] --
 * runs as ONE fused launch with hm_find's early exit (one stop word per
 * request), request r whole on device r mod ndev, round-robin
 * over that device's streams (HM_OPT_STREAMS, as hm_scan_many), and every
 * request of a chunk of 64 is enqueued on every device before the host waits
 * on any.  Of the window, the longest ascending run of digit segments that a
 * fused launch can hold is fused (all of it, but for chained layouts of more
 * than four final-block digits).  A request with no hit there whose range goes
 * on continues from the first nonce not fused through hm_find's per-segment
 * path, one request after another.  The host recomputes each hit's hash.
 *
 * n == 0 is HM_OK and enqueues nothing.  HM_ERR_INVALID: n < 0; n > 0 with
 * reqs, outs or found NULL; any request with msg == NULL and len > 0
 * (msg == NULL with len == 0 is the empty message).  Outputs are written only
 * on HM_OK, and all n are written or none.  An abandoned context returns
 * HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS applies to the whole call (auto: 2 s +
 * 8 x the sum of what hm_find's auto rule models for each request).
 * HM_OPT_FORCE_GENERIC and HM_OPT_GRID_PER_CU are honoured as the fused scan
 * launch honours them; HM_OPT_FUSED = 0 sends every request down the
 * per-segment path (the in-library A/B); the RCCL option does not apply.  Each
 * device keeps 64 word pairs, made on first use and kept until hm_close.  The
 * call changes nothing that hm_scan_stats*, hm_find_stats_sized,
 * hm_collect_stats_sized or hm_verify_stats_sized report. */
typedef struct hm_find_request {
    const uint8_t *msg;   /* borrowed for the call; may be NULL when len == 0 */
    size_t len;
    uint64_t lo, hi;      /* inclusive */
    uint64_t target;
} hm_find_request;

int hm_find_many(hm_ctx *ctx, const hm_find_request *reqs, int n, hm_result *outs, int *found);

/* The same answers on the host's cores, no GPU: hm_find_cpu request by
 * request (`threads` as there), under the same contract. */
int hm_find_many_cpu(const hm_find_request *reqs, int n, int threads, hm_result *outs,
                     int *found);

/* Work accounting of the most recent successful hm_find_many on a context.
 * The struct only grows at its end. */
typedef struct hm_find_many_stats {
    double wall_ms;           /* host wall time of the call                      */
    double kernel_ms;         /* summed HIP-event time of the fused find launches
                                 and of any fallback launches                    */
    uint64_t nonces_enqueued; /* as in hm_find_stats, summed over the batch      */
    uint64_t tasks_total;     /*   (a fused launch: its task ids)                */
    uint64_t tasks_run;
    int32_t requests;         /* n                                               */
    int32_t found;            /* requests with a hit                             */
    int32_t fused;            /* requests answered by their fused launch alone: a
                                 hit in it, or it covered [lo, hi]               */
    int32_t fallback;         /* requests that needed the per-segment path.  A
                                 request that enqueues nothing (lo > hi,
                                 target = 0) counts in neither                   */
    int32_t launches;         /* fused find launches plus fallback launches      */
    int32_t ndev;             /* devices of the context                          */
} hm_find_many_stats;
#define HM_FIND_MANY_STATS_SIZE_1_13 64 /* ABI 1.13 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_FIND_MANY_STATS_SIZE_1_13) of the last successful hm_find_many's
 * stats; HM_ERR_INVALID before the first one. */
int hm_find_many_stats_sized(const hm_ctx *ctx, hm_find_many_stats *out, size_t size);

/* ABI 1.11: share collection.  The result of
 *   for n = lo .. hi (inclusive): if Hash(msg, n) < target: emit (Hash, n)
 * *total = the number of such n, always exact (the whole range is always
 * hashed; strict '<' as in hm_find).
 *   *total <= cap: out[0 .. *total) holds every (Hash(msg, n), n), ascending
 *                  by nonce; nothing at or beyond out[*total] is touched.
 *   *total >  cap: out is not written at all.  The caller retries with
 *                  cap >= *total or a narrower range (the size-query idiom).
 *                  No "some cap of them" result is ever returned: the answer
 *                  never depends on dispatch order.
 *   cap == 0 with out == NULL is the pure count: the hit rate of the range at
 *   the target, what a server sets a share difficulty from.
 * target = 0 and lo > hi give *total = 0.  hi may be UINT64_MAX, and nonce
 * UINT64_MAX is an ordinary record.
 *
 * Arguments are validated as hm_find validates them; cap > HM_COLLECT_CAP_MAX,
 * cap > 0 with out == NULL, and total == NULL are HM_ERR_INVALID.  `out` and
 * `*total` are written only on HM_OK.  An abandoned context returns
 * HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS applies, HM_OPT_FORCE_GENERIC and
 * HM_OPT_GRID_PER_CU are honoured; the stream, fused and RCCL options do not
 * apply: every launch of every device is enqueued on stream 0 before the host
 * waits on any, the devices' shards are those of hm_partition (in pieces of
 * 2^40 nonces per device), and the host concatenates and sorts their records.
 * The host recomputes nothing: a record carries the hash the kernel formed.
 * Each device keeps a buffer of `cap` records (16 bytes each), grown when a
 * larger cap arrives and kept until hm_close.  hm_collect does not change what
 * hm_scan_stats* or hm_find_stats_sized report. */
#define HM_COLLECT_CAP_MAX (1u << 24) /* records; 256 MiB of device buffer per device */
int hm_collect(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
               uint64_t target, hm_result *out, size_t cap, uint64_t *total);

/* The same answer as hm_collect on the host's cores, no GPU (`threads` as
 * hm_scan_cpu's).  Each thread walks a contiguous chunk, ascending; the
 * chunks' records are concatenated in order. */
int hm_collect_cpu(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, uint64_t target,
                   int threads, hm_result *out, size_t cap, uint64_t *total);

/* Work accounting of the most recent successful hm_collect on a context.  The
 * struct only grows at its end. */
typedef struct hm_collect_stats {
    double wall_ms;    /* host wall time of the call                             */
    double kernel_ms;  /* HIP-event time from each device's first collect launch
                          to the end of its last, summed over devices            */
    uint64_t nonces;   /* nonces covered by the launches: hi - lo + 1            */
    uint64_t total;    /* the call's *total                                      */
    int32_t launches;  /* collect-kernel launches issued                         */
    int32_t ndev;      /* devices of the context                                 */
    int32_t overflow;  /* 1: *total > cap, `out` was not written; else 0         */
    int32_t reserved;
} hm_collect_stats;
#define HM_COLLECT_STATS_SIZE_1_11 48 /* ABI 1.11 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_COLLECT_STATS_SIZE_1_11) of the last successful collect's stats;
 * HM_ERR_INVALID before the first one. */
int hm_collect_stats_sized(const hm_ctx *ctx, hm_collect_stats *out, size_t size);

/* ABI 1.12: recheck a list.  The receiving side of share collection: a pool
 * hands out work at a share target and miners return lists of (hash, nonce)
 * records; the reference server believes them (server.go:273 only compares
 * the hash).  Two calls over one kernel that hashes a LIST of arbitrary
 * nonces, one per GPU lane, each with its own digit count:
 *
 *   hm_hash_many:  hashes[i] = Hash(msg, nonces[i]) for i < n.
 *   hm_verify:     record i is BAD iff
 *                      recs[i].hash != Hash(msg, recs[i].nonce)
 *                   or recs[i].hash >= target            (strict '<', as in find and collect)
 *
 * target = 0 makes every record bad.  target = UINT64_MAX checks the hash
 * alone, except that a record whose hash is UINT64_MAX is bad even when that
 * is its true hash.  Nonces may repeat, come in any order and have any digit
 * count 1..20; nonces 0 and UINT64_MAX are ordinary.  No range or duplicate
 * check is done: a caller does those on the host in one pass over the list.
 *
 * *bad = the number of bad records, always exact.  The size-query idiom of
 * the collect call applies:
 *   *bad <= cap: bad_idx[0 .. *bad) holds the indices of the bad records,
 *                ASCENDING; nothing at or beyond bad_idx[*bad] is touched.
 *   *bad >  cap: bad_idx is not written at all.
 *   cap == 0 with bad_idx == NULL is the pure count.
 * Only the count and the indices cross the bus back.  The hash-list call
 * writes all n hashes, or nothing if it does not return HM_OK.
 *
 * n == 0 returns HM_OK with *bad = 0 and enqueues nothing.  msg == NULL with
 * len == 0 is the empty message.  HM_ERR_INVALID: n > 0 with a NULL list,
 * hashes == NULL with n > 0, cap > HM_VERIFY_CAP_MAX, cap > 0 with
 * bad_idx == NULL, bad == NULL.  Outputs are written only on HM_OK.  An
 * abandoned context returns HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS applies (auto:
 * 2 s plus 8 x a per-record time, there being no range to model); no other
 * option does.  Both calls use stream 0 only and create no stream: the list is
 * cut contiguously across the context's devices in even shares, each share
 * into chunks of at most 2^22 elements (copy in, one launch, for hashes a copy
 * out), all devices' work is enqueued before the host waits on any, and the
 * host sums the counts and sorts the indices.  The caller's memory is not
 * registered or altered.  Each device keeps a chunk buffer (at most 64 MiB)
 * and a buffer of `cap` indices, made on first use, grown when needed and
 * kept until the context is closed.  Neither call changes what
 * hm_scan_stats*, hm_find_stats_sized or hm_collect_stats_sized report. */
#define HM_VERIFY_CAP_MAX (1u << 20) /* bad indices returned at most */
int hm_hash_many(hm_ctx *ctx, const uint8_t *msg, size_t len, const uint64_t *nonces, size_t n,
                 uint64_t *hashes);
int hm_verify(hm_ctx *ctx, const uint8_t *msg, size_t len, const hm_result *recs, size_t n,
              uint64_t target, uint64_t *bad_idx, size_t cap, uint64_t *bad);

/* The same answers on the host's cores, no GPU, under the same contract
 * (`threads` as hm_scan_cpu's; the compression too: x86 SHA extensions,
 * HM_CPU_NO_SHA=1 for portable C).  Each thread takes a contiguous part of
 * the list; the parts' bad indices are concatenated in order. */
int hm_hash_many_cpu(const uint8_t *msg, size_t len, const uint64_t *nonces, size_t n,
                     int threads, uint64_t *hashes);
int hm_verify_cpu(const uint8_t *msg, size_t len, const hm_result *recs, size_t n,
                  uint64_t target, int threads, uint64_t *bad_idx, size_t cap, uint64_t *bad);

/* Accounting of the most recent successful hm_hash_many or hm_verify on a
 * context (the hash-list call reports bad = 0).  The struct only grows at
 * its end. */
typedef struct hm_verify_stats {
    double wall_ms;    /* host wall time of the call                             */
    double kernel_ms;  /* summed HIP-event time of its launches                  */
    double copy_ms;    /* summed HIP-event time of its copies to and from the
                          device (the chunks in; for hashes, the chunks out)    */
    uint64_t records;  /* list elements: n                                       */
    uint64_t bad;      /* the call's *bad                                        */
    int32_t launches;  /* kernel launches issued (one per chunk)                 */
    int32_t ndev;      /* devices of the context                                 */
    int32_t overflow;  /* 1: *bad > cap, bad_idx was not written; else 0         */
    int32_t reserved;
} hm_verify_stats;
#define HM_VERIFY_STATS_SIZE_1_12 56 /* ABI 1.12 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_VERIFY_STATS_SIZE_1_12) of the last successful call's stats;
 * HM_ERR_INVALID before the first one. */
int hm_verify_stats_sized(const hm_ctx *ctx, hm_verify_stats *out, size_t size);

/* ABI 1.14: recheck the lists of many jobs.  hm_verify checks one message and
 * one list per blocking call; a pool sets its share target so that each
 * returned list is small, and serves many clients, so it holds many messages
 * at once.  hm_verify_many takes a batch of (message, list, target) requests
 * and answers all of them from as few launches as hold them: the message
 * changes INSIDE a launch.
 *
 *   bad_per_req[i] = the *bad that hm_verify(reqs[i]) returns, always exact.
 *   *bad           = the sum of the per-request counts.
 * Record k of request i is BAD iff
 *       recs[k].hash != Hash(msg_i, recs[k].nonce)  or  recs[k].hash >= target_i
 * -- 1.12's rule verbatim, target = 0 (every record bad) and target =
 * UINT64_MAX (the hash alone, but a hash of UINT64_MAX is bad) included.
 *
 * The size-query idiom, with ONE cap for the whole call:
 *   *bad <= cap: refs[0 .. *bad) holds every bad (request, index), ASCENDING by
 *                request and then by index (the index counts inside the
 *                request's list); nothing at or beyond refs[*bad] is touched.
 *   *bad >  cap: refs is not written at all.  The counts still are.
 *   cap == 0 with refs == NULL gives the pure counts.
 *
 * Requests may repeat a message, a list or a pointer; each is answered on its
 * own.  A request with n == 0 is legal and counts 0.  nreq == 0 is HM_OK with
 * *bad = 0 and enqueues nothing.  HM_ERR_INVALID: nreq < 0; nreq > 0 with
 * reqs or bad_per_req NULL; bad == NULL; cap > HM_VERIFY_CAP_MAX; cap > 0 with
 * refs == NULL; any request with msg == NULL and len > 0 (msg == NULL with
 * len == 0 is the empty message) or recs == NULL and n > 0.  Outputs are
 * written only on HM_OK, all of them or none.  An abandoned context returns
 * HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS applies to the whole call (auto:
 * hm_verify's rule over the summed record count); no other option does.
 *
 * Stream 0 only; no stream is created.  The concatenation of all requests'
 * records is cut contiguously across the context's devices in even shares by
 * record count (a cut may fall inside a request).  Each share is walked in
 * order and packed into launches: a launch closes when it holds 2^22 records
 * or 4096 jobs (a job: one request, or the piece of one that the launch
 * holds; a request is cut where a launch fills).  Per launch the host packs
 * the job table and the records into a pinned staging slot of the context and
 * issues ONE copy and ONE kernel launch; all devices' work is enqueued before
 * the host waits on any (beyond two launches per device it first waits for a
 * staging slot's copy), then the host sums the pieces' counts per request and
 * sorts the refs.  The caller's memory is neither registered nor altered.
 * Each device keeps two staging slots, a device copy of one, its count words
 * and a buffer of `cap` refs, made on first use, grown when needed and kept
 * until the context is closed.  The call changes nothing that hm_scan_stats*,
 * hm_find_stats_sized, hm_find_many_stats_sized, hm_collect_stats_sized or
 * hm_verify_stats_sized report.
 *
 * The packing pass is a host copy of every record: a caller with ONE large
 * list keeps hm_verify, which copies straight from the caller's memory. */
typedef struct hm_verify_request {
    const uint8_t *msg;     /* borrowed for the call; may be NULL when len == 0 */
    size_t len;
    const hm_result *recs;  /* borrowed for the call; may be NULL when n == 0 */
    size_t n;
    uint64_t target;
} hm_verify_request;

typedef struct hm_bad_ref {
    uint64_t request;  /* position of the request in reqs     */
    uint64_t index;    /* position of the bad record in its list */
} hm_bad_ref;          /* 16 bytes */

int hm_verify_many(hm_ctx *ctx, const hm_verify_request *reqs, int nreq,
                   uint64_t *bad_per_req, hm_bad_ref *refs, size_t cap, uint64_t *bad);

/* The same answers on the host's cores, no GPU, under the same contract
 * (`threads` and the compression as hm_verify_cpu's).  The flattened record
 * sequence is split over the threads; their counts and refs are concatenated
 * in order. */
int hm_verify_many_cpu(const hm_verify_request *reqs, int nreq, int threads,
                       uint64_t *bad_per_req, hm_bad_ref *refs, size_t cap, uint64_t *bad);

/* Accounting of the most recent successful hm_verify_many on a context.  The
 * struct only grows at its end. */
typedef struct hm_verify_many_stats {
    double wall_ms;    /* host wall time of the call                             */
    double kernel_ms;  /* summed HIP-event time of its launches                  */
    double copy_ms;    /* summed HIP-event time of its copies to the device      */
    uint64_t records;  /* summed record count of the requests                    */
    uint64_t bad;      /* the call's *bad                                        */
    uint64_t tasks;    /* tasks (64 records of one job) of those launches        */
    int32_t requests;  /* nreq                                                   */
    int32_t launches;  /* kernel launches issued                                 */
    int32_t copies;    /* host-to-device copies issued (one per launch)          */
    int32_t ndev;      /* devices of the context                                 */
    int32_t overflow;  /* 1: *bad > cap, refs was not written; else 0            */
    int32_t reserved;
} hm_verify_many_stats;
#define HM_VERIFY_MANY_STATS_SIZE_1_14 72 /* ABI 1.14 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_VERIFY_MANY_STATS_SIZE_1_14) of the last successful
 * hm_verify_many's stats; HM_ERR_INVALID before the first one. */
int hm_verify_many_stats_sized(const hm_ctx *ctx, hm_verify_many_stats *out, size_t size);

/* ABI 1.15: a batch of collects.  hm_collect makes one launch per digit
 * segment piece, on stream 0, one blocking call per message; a pool that hands
 * out small work units wants, per job, the shares below the share target (or,
 * with no buffer, the hit count a difficulty is set from) for many messages at
 * once.
 *
 *   totals[i] = the *total that hm_collect(reqs[i]) returns, always exact.
 *   *total    = the sum of the per-request totals.
 * Strict '<' as in hm_collect; target = 0 and lo > hi count 0; hi may be
 * UINT64_MAX, and nonce UINT64_MAX is an ordinary record.
 *
 * The size-query idiom, with ONE cap for the whole call (as hm_verify_many):
 *   *total <= cap: out[0 .. *total) holds every record, request-major:
 *                  request i's records start at totals[0] + ... + totals[i-1],
 *                  and inside a request they ascend by nonce, bit for bit what
 *                  hm_collect writes for that request.  Nothing at or beyond
 *                  out[*total] is touched.
 *   *total >  cap: out is not written at all.  totals and *total still are.
 *   cap == 0 with out == NULL gives the pure counts.
 *
 * Requests may repeat; each is answered on its own.  n == 0 is HM_OK with
 * *total = 0 and enqueues nothing.  HM_ERR_INVALID: n < 0; n > 0 with reqs or
 * totals NULL; total == NULL; cap > HM_COLLECT_CAP_MAX; cap > 0 with
 * out == NULL; any request with msg == NULL and len > 0 (msg == NULL with
 * len == 0 is the empty message).  Outputs are written only on HM_OK, all of
 * them or none.  An abandoned context returns HM_ERR_TIMEOUT.
 * HM_OPT_DEADLINE_MS applies to the whole call (auto: 2 s + 8 x the sum of what
 * hm_collect's auto rule models for each request).
 *
 * A request of at most 2^27 nonces whose digit segments all fit a fused launch
 * (all, but for chained layouts of more than four final-block digits) runs as
 * ONE launch of the fused collect kernel: request r whole on
 * device r mod ndev, round-robin over that device's streams (HM_OPT_STREAMS, as
 * hm_find_many), every request of a chunk of 64 enqueued on every device before
 * the host waits on any.  Each request has its own total word; the records of
 * a chunk's requests share the device's buffer and carry a request tag, and
 * the host groups them by tag and sorts each group by nonce.  Any other
 * request takes hm_collect's per-segment path WHOLE, one request after another
 * (there is no fused prefix: without an early exit it buys nothing).
 * HM_OPT_FORCE_GENERIC and HM_OPT_GRID_PER_CU are honoured as the fused scan
 * launch honours them; HM_OPT_FUSED = 0 sends every request down the
 * per-segment path (the in-library A/B); the RCCL option does not apply.  The
 * host recomputes nothing: a record carries the hash the kernel formed.  Each
 * device keeps hm_collect's record buffer (the two calls share it), a buffer
 * of `cap` 32-bit tags and 65 control words, made on first use, grown when a
 * larger cap arrives and kept until hm_close.  The call changes nothing that
 * any other *_stats* export reports.
 *
 * Measured per request against a loop of hm_collect (DESIGN.md §3f has the
 * rows): 64 requests over [0, 10^7] take 0.59 (an 8-byte message) and 0.36 (a
 * 120-byte one) of the loop's time, 64 requests over [0, 10^5] a third, a LONE
 * request over [0, 10^7] 0.85 and 0.78 (one launch that plans its whole range
 * first, against eight).  No measured row loses; a request of more than 2^27
 * nonces is hm_collect's own path at hm_collect's own time. */
typedef struct hm_collect_request {
    const uint8_t *msg;   /* borrowed for the call; may be NULL when len == 0 */
    size_t len;
    uint64_t lo, hi;      /* inclusive */
    uint64_t target;
} hm_collect_request;     /* 40 bytes, the shape of hm_find_request */

int hm_collect_many(hm_ctx *ctx, const hm_collect_request *reqs, int n, uint64_t *totals,
                    hm_result *out, size_t cap, uint64_t *total);

/* The same answers on the host's cores, no GPU: hm_collect_cpu request by
 * request (`threads` as there), under the same contract, the all-or-nothing
 * `out` included. */
int hm_collect_many_cpu(const hm_collect_request *reqs, int n, int threads, uint64_t *totals,
                        hm_result *out, size_t cap, uint64_t *total);

/* Work accounting of the most recent successful hm_collect_many on a context.
 * The struct only grows at its end. */
typedef struct hm_collect_many_stats {
    double wall_ms;    /* host wall time of the call                             */
    double kernel_ms;  /* summed HIP-event time of the fused collect launches and
                          of any fallback launches                               */
    uint64_t nonces;   /* nonces covered                                         */
    uint64_t total;    /* the call's *total                                      */
    uint64_t tasks;    /* task ids of the fused launches                         */
    int32_t requests;  /* n                                                      */
    int32_t fused;     /* requests answered by their fused launch alone          */
    int32_t fallback;  /* requests that took the per-segment path.  A request
                          that enqueues nothing (lo > hi, target = 0) counts in
                          neither                                                */
    int32_t launches;  /* fused collect launches plus fallback launches          */
    int32_t ndev;      /* devices of the context                                 */
    int32_t overflow;  /* 1: *total > cap, `out` was not written; else 0         */
} hm_collect_many_stats;
#define HM_COLLECT_MANY_STATS_SIZE_1_15 64 /* ABI 1.15 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_COLLECT_MANY_STATS_SIZE_1_15) of the last successful
 * hm_collect_many's stats; HM_ERR_INVALID before the first one. */
int hm_collect_many_stats_sized(const hm_ctx *ctx, hm_collect_many_stats *out, size_t size);

/* ABI 1.16: the next k shares.  A pool-style miner asks "from nonce lo, give
 * me the next k nonces below the target", over a range that is effectively
 * open.  Let H be the nonces n of the INCLUSIVE [lo, hi] with
 * Hash(msg, n) < target (strict '<', as in find and collect), ascending.
 *   *n = min(k, |H|), and out[0 .. *n) holds the *n LOWEST elements of H as
 *   (Hash(msg, n), n), ascending by nonce: bit for bit the first *n records
 *   hm_collect would write.  Nothing at or beyond out[*n] is touched.
 *   *n <  k: the range is exhausted, every nonce of it was hashed.
 *   *n == k: the caller resumes at out[k-1].nonce + 1.
 * k = 1 is hm_find (*n is its found).  target = 0 and lo > hi give *n = 0 and
 * enqueue nothing.  hi may be UINT64_MAX, and nonce UINT64_MAX is an ordinary
 * record.  The answer never depends on dispatch order.
 *
 * The call stops early inside a launch, as hm_find does, and records as
 * hm_collect does: waves append their hits to a device buffer
 * through one cursor; once the first k slots of it are all written, the largest
 * nonce among them becomes the device's stop word -- k hits at or below it
 * exist -- and waves skip every task above it.  The host enqueues launches in
 * ascending order on stream 0, at most four in flight, reads the words back
 * after each batch, never issues work above the lowest stop word of any device,
 * and ends the call when nothing unissued lies below it.  It then sorts the
 * records by nonce and keeps the k lowest, after hm_collect's checks.  With
 * several devices each seeks k hits in its own shard (hm_find's pieces) and the
 * host merges the union.  The device buffer holds min(2^24, 2k + 4096) records;
 * when a dense target overflows it the early exit has still bounded the answer,
 * and the call takes it exactly from hm_collect's path over ascending windows
 * of the bounded range (hm_find_k_stats.fallback = 1).
 *
 * HM_ERR_INVALID: k == 0, k > HM_FIND_K_MAX, out or n NULL, msg == NULL with
 * len > 0 (msg == NULL with len == 0 is the empty message).  `out` and `*n` are
 * written only on HM_OK.  An abandoned context returns HM_ERR_TIMEOUT.
 * HM_OPT_DEADLINE_MS applies (auto models the whole range, as for hm_find: an
 * upper bound), HM_OPT_FORCE_GENERIC and HM_OPT_GRID_PER_CU are honoured; the
 * stream, fused and RCCL options do not apply.  The records go through
 * hm_collect's device buffer, and each device keeps five more words, made on
 * first use and kept until hm_close.  The call changes nothing that any other
 * hm_*_stats* call reports. */
#define HM_FIND_K_MAX (1u << 20)
int hm_find_k(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
              uint64_t target, size_t k, hm_result *out, size_t *n);

/* The same answer as hm_find_k on the host's cores, no GPU (`threads` and
 * windows as hm_find_cpu's).  Threads keep the hits of the windows they walk;
 * once k are held, windows above the largest of the k lowest are not begun. */
int hm_find_k_cpu(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, uint64_t target,
                  size_t k, int threads, hm_result *out, size_t *n);

/* Work accounting of the most recent successful hm_find_k on a context.  The
 * struct only grows at its end. */
typedef struct hm_find_k_stats {
    double wall_ms;           /* host wall time of the call                      */
    double kernel_ms;         /* summed HIP-event time of its launches, the
                                 overflow path's collect launches included       */
    uint64_t nonces_enqueued; /* as in hm_find_stats, plus the overflow path's
                                 windows                                         */
    uint64_t tasks_total;     /* tasks of the find_k launches issued             */
    uint64_t tasks_run;       /* tasks whose hash loop ran (the others were
                                 skipped above the stop word)                    */
    uint64_t records;         /* records read back from the devices' buffers
                                 (min(cursor, buffer) summed over devices)       */
    int32_t launches;         /* find_k launches plus overflow-path launches     */
    int32_t ndev;             /* devices of the context                          */
    int32_t found;            /* the call's *n                                   */
    int32_t fallback;         /* 1: a device's buffer overflowed and the answer
                                 came from the overflow path; else 0             */
} hm_find_k_stats;
#define HM_FIND_K_STATS_SIZE_1_16 64 /* ABI 1.16 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_FIND_K_STATS_SIZE_1_16) of the last successful hm_find_k's stats;
 * HM_ERR_INVALID before the first one. */
int hm_find_k_stats_sized(const hm_ctx *ctx, hm_find_k_stats *out, size_t size);

/* ABI 1.17: a batch of hm_find_k calls.  A pool-style caller holds many jobs,
 * usually one message per client, and wants the next k shares of each; at the
 * targets such callers use hm_find_k is bound by its launches and host round
 * trips, so a loop over it is too.
 *   off_i = the sum of reqs[j].k for j < i; request i owns out[off_i .. off_i +
 *   k_i).  counts[i] and out[off_i .. off_i + counts[i]) are exactly what
 *   hm_find_k(reqs[i]) returns in *n and out, bit for bit, ascending by nonce.
 *   Nothing at or beyond out[off_i + counts[i]] inside the request's slot is
 *   touched.  counts[i] < k_i: that request's range is exhausted.
 * target = 0 and lo > hi give 0 and enqueue nothing.  hi may be UINT64_MAX, and
 * nonce UINT64_MAX is an ordinary record.  n == 0 is HM_OK and enqueues nothing.
 * Outputs are written only on HM_OK, all n requests or none.  The answer never
 * depends on dispatch order.
 *
 * Each request's first 2^27 nonces run as ONE fused launch that records as
 * hm_find_k does and exits early: the request has its own five
 * control words and its own slice of min(2^24, 2k + 4096) records, request r
 * goes whole to device r mod ndev and round-robins over that device's streams,
 * and every request of a chunk (at most 64 requests, and at most 2^24 records
 * of slices per device) is enqueued on every device before the host waits on
 * any.  A request whose window holds fewer than k hits and whose range goes on
 * continues from the first nonce not fused through hm_find_k's per-segment
 * path, for the hits still missing; one whose launch overran its slice takes
 * that path whole.
 *
 * HM_ERR_INVALID: n < 0; n > 0 with reqs, out or counts NULL; a request with
 * k == 0 or k > HM_FIND_K_MAX, or with msg == NULL and len > 0 (msg == NULL
 * with len == 0 is the empty message).  An abandoned context returns
 * HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS covers the whole call; HM_OPT_FORCE_GENERIC,
 * HM_OPT_GRID_PER_CU and HM_OPT_STREAMS are honoured as in hm_find_many;
 * HM_OPT_FUSED = 0 sends every request down the per-segment path.  The slices
 * share hm_collect's device buffer, and each device keeps 64 x 5 more words,
 * made on first use and kept until hm_close.  The call changes nothing that any
 * other hm_*_stats* call reports. */
typedef struct hm_find_k_request {
    const uint8_t *msg; size_t len;   /* msg may be NULL when len == 0 */
    uint64_t lo, hi;                  /* inclusive */
    uint64_t target;
    size_t k;                         /* 1 .. HM_FIND_K_MAX */
} hm_find_k_request;

int hm_find_k_many(hm_ctx *ctx, const hm_find_k_request *reqs, int n, hm_result *out,
                   size_t *counts);

/* The same answers on the host's cores, no GPU: hm_find_k_cpu request by
 * request; all outputs are written, or none. */
int hm_find_k_many_cpu(const hm_find_k_request *reqs, int n, int threads, hm_result *out,
                       size_t *counts);

/* Work accounting of the most recent successful hm_find_k_many on a context.
 * The struct only grows at its end. */
typedef struct hm_find_k_many_stats {
    double wall_ms;           /* host wall time of the call                      */
    double kernel_ms;         /* summed HIP-event time of its launches           */
    uint64_t nonces_enqueued; /* nonces of the launches issued                   */
    uint64_t tasks_total;     /* tasks of those launches                         */
    uint64_t tasks_run;       /* tasks whose hash loop ran (the others were
                                 skipped above a stop word)                      */
    uint64_t records;         /* records read back from the devices              */
    uint64_t found;           /* the sum of counts                               */
    int32_t requests;         /* n                                               */
    int32_t fused;            /* requests answered by their fused launch alone   */
    int32_t fallback;         /* requests that needed the per-segment path for
                                 any reason.  A request that enqueues nothing
                                 (lo > hi, target = 0) counts in neither         */
    int32_t overflow;         /* of those, requests whose fused launch overran
                                 its slice                                       */
    int32_t launches;         /* fused launches plus fallback launches           */
    int32_t ndev;             /* devices of the context                          */
} hm_find_k_many_stats;
#define HM_FIND_K_MANY_STATS_SIZE_1_17 80 /* ABI 1.17 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_FIND_K_MANY_STATS_SIZE_1_17) of the last successful
 * hm_find_k_many's stats; HM_ERR_INVALID before the first one. */
int hm_find_k_many_stats_sized(const hm_ctx *ctx, hm_find_k_many_stats *out, size_t size);

/* ---------------------------------------------------------------------------
 * hm_cancel (ABI 1.18): stop an in-flight find from another thread -- "the job
 * changed".
 *
 * May be called from any thread while another thread is inside a call on `ctx`.
 * It does not take the context's mutex, makes no HIP call and returns at once:
 *   1               an hm_find, hm_find_k, hm_find_many or hm_find_k_many call
 *                   was in flight on ctx and has been signalled
 *   0               nothing cancellable was in flight: no call at all, a call of
 *                   another family, or an abandoned context.  Nothing is
 *                   remembered: a later call is not affected (a cancel meant for
 *                   the old job never kills the new one)
 *   HM_ERR_INVALID  ctx == NULL
 * Racing hm_close with hm_cancel is the caller's error, as racing hm_close with
 * any other call is.
 *
 * A signalled call has one of two outcomes, nothing else:
 *   HM_ERR_CANCELLED  no output is written (out, found, n, counts untouched, as
 *                     for any error).  The context is fully usable: every launch
 *                     the call queued has ended, the next call of any family
 *                     answers exactly, and no hm_*_stats record of the cancelled
 *                     family has moved
 *   HM_OK             its exact answer, when that was already in hand when the
 *                     call first observed the signal (or it never did)
 * The signal reaches the GPU inside a running launch: one wave of each
 * find-family launch relays the context's cancel flag (pinned host memory) to
 * the launch's stop word, and the kernels' own early exit ends the launch and
 * every launch queued behind it.  HM_OPT_DEADLINE_MS is
 * unchanged: it remains the fence for a hung GPU and still abandons the context.
 *
 * NOT cancellable in this version: hm_scan*, hm_collect*, hm_verify* and
 * hm_hash_many.  They are bounded by their range or list and enqueue everything
 * up front; hm_cancel returns 0 while one runs and it finishes normally.  The
 * _cpu calls take no context and cannot be cancelled.
 * ------------------------------------------------------------------------- */
int hm_cancel(hm_ctx *ctx);

#define HM_CANCEL_FAMILY_NONE 0
#define HM_CANCEL_FAMILY_FIND 1
#define HM_CANCEL_FAMILY_FIND_K 2
#define HM_CANCEL_FAMILY_FIND_MANY 3
#define HM_CANCEL_FAMILY_FIND_K_MANY 4

/* Cancellation accounting of a context since hm_open.  The struct only grows
 * at its end. */
typedef struct hm_cancel_stats {
    double latency_ms;          /* the last call that returned HM_ERR_CANCELLED:
                                   from hm_cancel's flag store to that call's
                                   return (0 before the first one)                */
    uint64_t cancels;           /* hm_cancel calls that returned 1                */
    uint64_t cancelled_calls;   /* calls that returned HM_ERR_CANCELLED           */
    int32_t launches_in_flight; /* of that last call: launches in flight when the
                                   host first saw the signal                      */
    int32_t family;             /* of that last call: HM_CANCEL_FAMILY_*          */
} hm_cancel_stats;
#define HM_CANCEL_STATS_SIZE_1_18 32 /* ABI 1.18 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_CANCEL_STATS_SIZE_1_18).  Like hm_cancel it does not take the
 * context's mutex; all zeros before the first hm_cancel. */
int hm_cancel_stats_sized(const hm_ctx *ctx, hm_cancel_stats *out, size_t size);

/* ---------------------------------------------------------------------------
 * hm_scan_k (ABI 1.19): the k lowest hashes of a range in one pass -- the
 * runner-ups of a round, the best k shares, the winner audited against the
 * next-best.  The reference's loop (miner.go:46-59) is k = 1.
 *
 *   *n = min(k, number of nonces in the inclusive [lo, hi])
 *   out[0 .. *n) holds the *n lexicographically smallest (Hash(msg, nonce),
 *   nonce) pairs of the range, ascending in that order: ties in the hash go
 *   to the lower nonce, as in hm_scan.  Nothing at or beyond out[*n] is
 *   touched.  On a non-empty range out[0] is bit for bit hm_scan's answer.
 *
 * lo > hi gives *n = 0 and leaves `out` unwritten.  Every nonce is eligible,
 * UINT64_MAX included.  The whole range is always hashed: there is no target
 * and no early exit, and the answer never depends on dispatch order.
 *
 * HM_ERR_INVALID: k == 0, k > HM_SCAN_K_MAX, out or n NULL, msg == NULL with
 * len > 0.  `out` and `*n` are written only on HM_OK.  An abandoned context
 * returns HM_ERR_TIMEOUT.  HM_OPT_DEADLINE_MS applies as it does for
 * hm_collect; HM_OPT_FORCE_GENERIC and HM_OPT_GRID_PER_CU are honoured; the
 * stream, fused and RCCL options do not apply.  The call is not cancellable:
 * hm_cancel returns 0 while it runs, as for hm_scan and hm_collect.
 *
 * Every launch of every device is enqueued on its stream 0 before the host
 * waits on any, each followed by a small fold launch that merges the
 * launch's per-wave lists into the device's list of k; the devices' shards
 * are hm_collect's.  The host merges the devices' lists and rechecks every
 * record it returns (hash recomputed, nonce in range, order strict): a
 * record that fails is HM_ERR_INTERNAL.  Each device keeps a 16 MiB wave-list
 * buffer, made on the first hm_scan_k and kept until hm_close.  For k >
 * HM_SCAN_K_MAX use hm_collect at a target.  hm_scan_k does not change what
 * any other family's stats call reports. */
#define HM_SCAN_K_MAX 32u
int hm_scan_k(hm_ctx *ctx, const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi,
              uint32_t k, hm_result *out, size_t *n);

/* The same answer as hm_scan_k on the host's cores, no GPU (`threads` as
 * hm_scan_cpu's; 0 = the hardware threads).  Each thread keeps the k lowest
 * of its contiguous chunk; the lists are merged at the end. */
int hm_scan_k_cpu(const uint8_t *msg, size_t len, uint64_t lo, uint64_t hi, uint32_t k,
                  int threads, hm_result *out, size_t *n);

/* Work accounting of the most recent successful hm_scan_k on a context.  The
 * struct only grows at its end. */
typedef struct hm_scan_k_stats {
    double wall_ms;       /* host wall time of the call                          */
    double kernel_ms;     /* HIP-event time from each device's first launch to
                             the end of its last fold, summed over devices       */
    uint64_t nonces;      /* nonces covered by the launches: hi - lo + 1         */
    uint64_t inserted;    /* device-side: records that passed a wave's bound and
                             entered its list, summed at wave exit.  Far below
                             `nonces` on a large range: the bound at work        */
    uint64_t compactions; /* device-side: list compactions of the scan waves,
                             each wave's last one included                       */
    int32_t launches;     /* scan_k-kernel launches issued (each has one fold)   */
    int32_t ndev;         /* devices of the context                              */
    int32_t k;            /* the call's k                                        */
    int32_t count;        /* the call's *n                                       */
} hm_scan_k_stats;
#define HM_SCAN_K_STATS_SIZE_1_19 56 /* ABI 1.19 */

/* Writes at most `size` bytes (pass sizeof the struct as the caller compiled
 * it; >= HM_SCAN_K_STATS_SIZE_1_19) of the last successful hm_scan_k's stats;
 * HM_ERR_INVALID before the first one. */
int hm_scan_k_stats_sized(const hm_ctx *ctx, hm_scan_k_stats *out, size_t size);

int hm_set_option(hm_ctx *ctx, int opt, int64_t value);

const char *hm_strerror(int rc);

void hm_close(hm_ctx *ctx);

/* ABI version: (major << 16) | minor. */
int hm_version(void);

/* Build identity (ABI 1.6): 16 hex digits of sha256 over the sources the
 * library was built from (distributed_bitcoinminer_amd/build_id.py: csrc/,
 * this header and hipminer_debug.h, by path and content).  A caller holding the source tree can
 * check that the loaded library is that tree's build.  Static storage. */
const char *hm_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* HIPMINER_H */
