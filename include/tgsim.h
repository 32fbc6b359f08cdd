/*
 * tgsim.h — C ABI of the MI355X network-emulation engine (libtgsim.so).
 *
 * This is the drop-in boundary for testground's per-packet enforcement of the sidecar's
 * network.Config.  In the reference the sidecar programs the Linux kernel (HTB + netem + FIB)
 * through netlink; every call below replaces one of those netlink/kernel interactions:
 *
 *   tgsim_configure   <- sidecar.Network.ConfigureNetwork       pkg/sidecar/instance.go:37-42
 *                        DockerNetwork.ConfigureNetwork         pkg/sidecar/docker_network.go:51-148
 *                          (network-name check :52-55, routing policy :57 -> route.go:102-117,
 *                           Enable=false disconnect :65-75, IP change :77-88,
 *                           link.Shape :139 -> link.go:155-183, link.AddRules :143 -> link.go:187-217)
 *   tgsim_submit/step <- the kernel data path the sidecar configured: FIB lookup of the
 *                        blackhole/prohibit routes (link.go:189-211), HTB class 1:2 token bucket
 *                        (link.go:118-128, :156-167), netem leaf 2:0 (link.go:131-141, :169-179)
 *   tgsim_drain       <- veth -> docker bridge -> peer delivery (pkg/runner/local_docker.go:706-721)
 *   tgsim_signal/
 *   tgsim_barrier     <- sync-service SignalEntry / SignalAndWait used by the handler
 *                        (pkg/sidecar/sidecar_handler.go:40-44, :75-80); the counters live in
 *                        device memory (K7), mirrored to pinned host memory for polling
 *   TGSIM_OPT_K8S     <- K8sNetwork.ConfigureNetwork instead of DockerNetwork's
 *                        (pkg/sidecar/k8s_network.go:114-256)
 *
 * A Go maintainer binds these with cgo.  Rules of the ABI:
 *   - plain C structs, caller-owned buffers, no exceptions across the boundary;
 *   - every int-returning call returns 0 (or a count) on success and a negative errno value on
 *     failure; tgsim_last_error() then describes the failure;
 *   - one engine handle owns its HIP stream and device memory and is NOT re-entrant: a host that
 *     calls from several goroutines/threads funnels the calls through one owner (the reference
 *     handler calls ConfigureNetwork sequentially per instance, concurrently across instances,
 *     sidecar_handler.go:26,:71 and pkg/docker/manager.go:166-177).
 *
 * Per-packet semantics (units, decision order, Philox keying, tie-breaks) are specified in
 * DESIGN.md §3 and restated independently by the CPU oracle in oracle/tgoracle.c.
 */
#ifndef TGSIM_H
#define TGSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGSIM_ABI_VERSION 2u

/* Reserved destination id: traffic leaving the data network (the "external" routes that
 * RoutingPolicy AllowAll/DenyAll adds or removes, route.go:68-117). */
#define TGSIM_EXTERNAL 0xFFFFFFFFu

/* network.FilterAction (sdk-go; used at link.go:194-209). */
enum tgsim_filter { TGSIM_ACCEPT = 0, TGSIM_REJECT = 1, TGSIM_DROP = 2 };

/* network.RoutingPolicyType (route.go:106-112).  UNSET behaves as DenyAll (default case :110). */
enum tgsim_policy { TGSIM_POLICY_UNSET = 0, TGSIM_ALLOW_ALL = 1, TGSIM_DENY_ALL = 2 };

/* Per-packet verdict codes (low nibble: the offered packet; high nibble: its netem clone). */
enum tgsim_verdict {
    TGSIM_V_SCHEDULED = 0,    /* passed netem+HTB, delivered at tgsim_delivery.t_ns          */
    TGSIM_V_DISCONNECTED = 1, /* src or dst has Enable=false (docker_network.go:65-75)        */
    TGSIM_V_NO_ROUTE = 2,     /* external dst while routing policy != AllowAll (route.go:110) */
    TGSIM_V_BLACKHOLE = 3,    /* LinkRule Drop -> blackhole route, sender sees EINVAL         */
    TGSIM_V_PROHIBIT = 4,     /* LinkRule Reject -> prohibit route, sender sees EACCES        */
    TGSIM_V_LOSS = 5,         /* netem loss event                                             */
    TGSIM_V_QUEUE_FULL = 6,   /* netem limit (1000 packets) reached                           */
    TGSIM_V_EXTERNAL = 7,     /* external dst with AllowAll: leaves the data network unshaped */
    TGSIM_V_NONE = 15         /* (high nibble) no clone was made                              */
};

/* Delivery flags. */
#define TGSIM_FLAG_DUP 0x1u     /* this record is the netem clone of the offered packet */
#define TGSIM_FLAG_CORRUPT 0x2u /* netem corrupt event fired                          */

/* Engine flags (tgsim_opts.flags). */
#define TGSIM_OPT_KEEP_DELIVERIES 0x1u /* keep delivered records for tgsim_drain (default on via 0) */
#define TGSIM_OPT_DISCARD_DELIVERIES 0x2u /* bench: sort deliveries but do not accumulate them  */
#define TGSIM_OPT_METRICS 0x4u            /* per-instance counters and histograms (tgsim_metrics) */
/* K8sNetwork semantics (k8s_network.go:114-256) instead of DockerNetwork's (docker_network.go:51-148):
 * only network "default" (else "configured network is not `default`"); the first call re-creates
 * the data link (InitializeNetwork, :85-112); Shape -> AddRules -> routing policy, the policy only
 * on an enabled network (:246-254); connecting with an IPv6 address fails "ipv6 not supported"
 * (:161-163), after an address change has already disconnected the instance (:142-155). */
#define TGSIM_OPT_K8S 0x8u

typedef struct {
    uint32_t abi_version;  /* = TGSIM_ABI_VERSION                                          */
    uint32_t n_peers;      /* simulated instances in the whole run (all shards)            */
    uint32_t shard_begin;  /* sources owned by this engine: [shard_begin, shard_end)       */
    uint32_t shard_end;    /* 0/0 -> [0, n_peers)                                          */
    uint64_t seed;         /* Philox4x32-10 key                                            */
    uint64_t tick_ns;      /* simulation tick; 0 -> 1000 ns                                */
    uint32_t queue_limit;  /* netem limit; 0 -> 1000 (netlink default); max 1024          */
    uint32_t flags;        /* TGSIM_OPT_*                                                  */
    uint64_t lookahead_ns; /* HTB horizon beyond the step end (closed-loop drivers); 0 = none */
    uint32_t subnet_base;  /* data-network base address, host order; 0 -> 16.0.0.0          */
    int32_t device;        /* HIP device ordinal; -1 -> current device                       */
} tgsim_opts;

/* One LinkRule (network.LinkRule{LinkShape.Filter, Subnet}); only Filter is honoured, exactly as
 * in the reference (link.go:185-186). */
typedef struct {
    uint32_t prefix; /* IPv4 network address, host byte order */
    uint8_t len;     /* prefix length 0..32                    */
    uint8_t action;  /* enum tgsim_filter                      */
    uint16_t _pad;
} tgsim_rule;

/* network.LinkShape as the reference passes it to netlink (link.go:155-183). */
typedef struct {
    int64_t latency_ns;     /* time.Duration */
    int64_t jitter_ns;      /* time.Duration */
    uint64_t bandwidth_bps; /* bits/s; 0 = unlimited (link.go:156-159) */
    float loss, corrupt, corrupt_corr, reorder, reorder_corr, duplicate, duplicate_corr; /* percent */
    uint32_t _pad;
} tgsim_shape;

/* network.Config flattened (sdk-go; fields used at docker_network.go:52-143, k8s_network.go:114-254).
 * cfg.IPv4 / cfg.IPv6 are pointers in sdk-go (nil = keep the current address); has_ipv4 /
 * has_ipv6 carry that.  A changed address (docker_network.go:77-78) disconnects and reconnects the
 * instance: its netem/HTB qdiscs are re-created empty and packets still queued towards it at any
 * sender are lost (they leave the sender and find no port).  LinkRule subnets are IPv4 only: an
 * IPv6 rule subnet must be rejected by the binding, never truncated. */
typedef struct {
    const char* network;    /* must be "default" (else "unsupported network: %s") */
    uint8_t enable;
    uint8_t routing_policy; /* enum tgsim_policy */
    uint8_t has_ipv4;
    uint8_t has_ipv6;
    uint32_t ipv4;          /* host order; used when has_ipv4 */
    tgsim_shape shape;      /* cfg.Default */
    const tgsim_rule* rules;
    uint32_t n_rules;
    uint32_t _pad2;
    uint8_t ipv6[16];       /* network order; used when has_ipv6 */
} tgsim_config;

/* Offered packet, host -> engine (16 B). tick is relative to the engine's current time and must
 * be < the n_ticks of the next tgsim_step.  seq is the per-source sequence number that keys the
 * Philox stream together with (seed, src, dst). */
typedef struct {
    uint32_t src;
    uint32_t dst; /* peer id or TGSIM_EXTERNAL */
    uint32_t seq;
    uint16_t len; /* bytes on the wire */
    uint16_t tick;
} tgsim_pkt;

/* Delivered packet, engine -> host (24 B).  Drain order: (dst, t_ns, src, seq, clone first). */
typedef struct {
    uint64_t t_ns; /* delivery time (HTB departure) */
    uint32_t src;
    uint32_t dst;
    uint32_t seq;
    uint16_t len;
    uint16_t flags; /* TGSIM_FLAG_* */
} tgsim_delivery;

typedef struct {
    uint64_t offered;         /* offered packets processed (originals)            */
    uint64_t scheduled;       /* records given a delivery time (clones included)  */
    uint64_t cloned;          /* netem duplicates created                        */
    uint64_t corrupted;       /* corrupt events on scheduled records             */
    uint64_t by_verdict[8];   /* originals+clones per enum tgsim_verdict         */
    uint64_t bytes_scheduled; /* sum of len over scheduled records               */
    uint64_t now_tick;        /* engine time after the last step                 */
    uint64_t queue_state_bytes; /* netem queue state carried across steps: 16 B per
                                   queued item + 8 B per departing item, summed at
                                   every step start and end (the HBM round trip)   */
    uint64_t flushed;         /* queued/departing items lost when their sender's data
                                 link was removed (disconnect, re-addressing)       */
    uint64_t lost_in_flight;  /* records served by HTB whose destination had been
                                 disconnected or re-addressed after they were
                                 queued (no delivery)                               */
} tgsim_stats_t;

/* Closed-loop gossip flood workload, generated and consumed on the device.
 * Flood f (0 <= f < n_floods) starts at tick start_tick + f * start_gap_ticks at its origin peer;
 * every peer forwards a flood once, on its first receipt, to its `degree` out-neighbours
 * (a fixed hash of (seed, peer, k)), one msg_len-byte packet each, seq = f * degree + k, offered
 * at the tick after the receipt's delivery time.  Corrupted deliveries are not receipts.
 * Flood starts and receipts are 32-bit ticks: tgsim_gossip_init returns -EINVAL when the last flood's
 * start tick, start_tick + (n_floods - 1) * start_gap_ticks, exceeds 0xFFFFFFFE, and tgsim_gen_gossip
 * -EOVERFLOW when its window ends beyond tick 0xFFFFFFFE (a receipt later than that saturates there). */
typedef struct {
    uint32_t n_floods;         /* 1..64                                                      */
    uint32_t degree;           /* out-neighbours per peer, 1..64                             */
    uint32_t msg_len;          /* bytes per message, 1..65535                                */
    uint32_t start_gap_ticks;  /* ticks between flood starts                                 */
    uint64_t start_tick;       /* absolute tick of flood 0 (>= the engine's next window)     */
} tgsim_gossip;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int tgsim_create(const tgsim_opts* opts, void** out_engine);
void tgsim_destroy(void* engine);
const char* tgsim_last_error(const void* engine);
uint32_t tgsim_abi_version(void);

/* ---- configuration (replaces netlink: Shape / AddRules / routing policy / connect) --------- */
/* Applies cfg to instance `peer` at the engine's current time (effective for packets offered in
 * the next step).  Follows DockerNetwork.ConfigureNetwork's order of operations.  Every shard of a
 * multi-GPU run must receive every call (peer tables are replicated). */
int tgsim_configure(void* engine, uint32_t peer, const tgsim_config* cfg);
/* n tgsim_configure calls in order (cfgs[i] to peers[i]): the Go host funnels the per-instance
 * ConfigureNetwork calls into one engine goroutine, which drains its queue in one batch.
 * rcs[i] (optional) receives each call's return code; returns the number of failed calls. */
int64_t tgsim_configure_batch(void* engine, const uint32_t* peers, const tgsim_config* cfgs, size_t n,
                              int32_t* rcs);
/* How many times `peer`'s data link has been removed so far: a disconnect (Enable=false,
 * docker_network.go:65-75) or a re-addressing reconnect (:77-88; k8s_network.go:130-155).  A caller
 * that holds state about packets in flight (the packet bridge) compares it before and after a
 * tgsim_configure: a changed value means every packet queued by the peer, or towards it, is gone
 * (tgsim_stats_t.flushed / lost_in_flight) and will never be delivered. */
int64_t tgsim_link_generation(void* engine, uint32_t peer);

/* ---- data path ---------------------------------------------------------------------------- */
int tgsim_submit(void* engine, const tgsim_pkt* pkts, size_t n);
/* Storm-style synthetic traffic generated on the device for the next step:
 * per source and tick Poisson(lambda) packets to a uniform destination != src, len U{64..1500}. */
int tgsim_gen_storm(void* engine, double lambda, uint32_t n_ticks);
/* Advances time by n_ticks: every offered packet of the window goes through filter -> netem ->
 * HTB; deliveries are routed to their destination and sorted.  Single-shard convenience.
 * On an engine that owns every peer the step is asynchronous on the engine's stream (with
 * TGSIM_OPT_DISCARD_DELIVERIES and no gossip driver it returns without a host round trip); every
 * call that reads results (drain, verdicts, stats, gossip_reached, sim_kernel_ms) synchronizes
 * first.  A simulated-time overflow (-EOVERFLOW) is then reported by the next step or reader.
 * Simulated-time overflow: any eligibility time (offer time + netem delay) or departure time (HTB's,
 * the t_ns of the delivery record) at or beyond 2^46 ns (19.5 simulated hours), whatever tick_ns is;
 * the window's results are not handed out and the error is sticky: from the reader of that window
 * on, every step and every reader (drain, verdicts, stats, sync, the reports) returns -EOVERFLOW.  A window may end beyond 2^46 ns as long as no packet's times do. */
int tgsim_step(void* engine, uint32_t n_ticks);
/* n_steps consecutive tgsim_step(engine, n_ticks) calls, with identical results (verdicts then
 * refer to the last window).  Windows of generated traffic (tgsim_gen_storm) on an engine that owns
 * every peer run in launches of up to TGSIM_FUSE windows (default and most: kFuseMax = 32; a longer
 * call ends with a short launch of 6 where that shortens the wait after it), fewer per launch when their buffers would take more
 * than half of the free device memory (TGSIM_FUSE_MEM_MB sets that budget): a source's next window starts as soon as its previous one
 * is done, so one window's slowest sources overlap the next window's first ones (no launch tail or
 * gap between the windows of a group).  A source whose previous window does not complete in time
 * (a hardware fault) is reported as -EIO. */
int tgsim_step_n(void* engine, uint32_t n_ticks, uint32_t n_steps);

/* Multi-shard form of tgsim_step.  Phase 1 simulates the owned sources and writes the scheduled
 * records into d_out (DEVICE memory, caller-owned, capacity out_cap records) grouped by the
 * destination's shard; rank_bounds[0..n_ranks] are the peer boundaries of the shards and
 * rank_counts[0..n_ranks-1] receives the per-shard record counts (host memory).  Returns once
 * d_out is complete and every earlier delivery (tgsim_deliver_async) has finished. */
int tgsim_step_sim(void* engine, uint32_t n_ticks, uint32_t n_ranks, const uint32_t* rank_bounds,
                   void* d_out, size_t out_cap, uint64_t* rank_counts);
/* tgsim_step_sim in two halves, so a host can start the next step's simulation before it
 * exchanges this step's records: _launch enqueues the simulation and the routing into d_out and
 * returns; _finish waits for the oldest launched step (and for earlier asynchronous deliveries)
 * and fills its counts.  Up to two launched steps may be pending (each with its own d_out), so the
 * simulate stream always has the next step queued; tgsim_step and tgsim_step_sim refuse (-EBUSY)
 * while any is.  Records beyond out_cap are dropped and reported as -ENOSPC by _finish. */
int tgsim_step_sim_launch(void* engine, uint32_t n_ticks, uint32_t n_ranks, const uint32_t* rank_bounds,
                          void* d_out, size_t out_cap);
int tgsim_step_sim_finish(void* engine, uint64_t* rank_counts);
/* tgsim_step_sim_finish without the wait for earlier asynchronous deliveries: the caller orders
 * the reuse of a delivery's input buffer on the device instead (tgsim_delivery_event), so the host
 * never blocks on the delivery stream. */
int tgsim_step_sim_counts(void* engine, uint64_t* rank_counts);
/* Slotted form of the pipelined step, for an exchange with fixed per-rank sizes (no count
 * exchange, so the host never waits for the device): d_out holds n_ranks chunks of
 * (slot_cap + 1) records; chunk r starts with a header record whose t_ns is the number of records
 * for rank r that follow it.  routed_event (a hipEvent_t, may be null) is recorded when d_out is
 * complete; the exchange waits for it on the device.  A rank whose records exceed slot_cap sets a
 * sticky error: the next step launch, release or reader fails with -ENOSPC.  _release retires the
 * oldest launched step without waiting for it. */
int tgsim_step_sim_launch_slotted(void* engine, uint32_t n_ticks, uint32_t n_ranks, const uint32_t* rank_bounds,
                                  void* d_out, uint64_t slot_cap, void* routed_event);
int tgsim_step_sim_release(void* engine);
/* Fused form of the slotted step (n_win generated windows in one launch, tgsim_step_n): d_out holds
 * n_ranks x n_win chunks of (slot_cap + 1) records, rank-major (chunk r * n_win + w: window w's
 * records for rank r behind its count header), so one all-to-all moves the whole group; counts as
 * ONE launched step for _release.  -EINVAL when the next n_win windows are not fusable; on an engine
 * with TGSIM_OPT_METRICS or an armed group matrix no windows are (n_win >= 2 is refused, naming that
 * reason, before anything is simulated). */
int tgsim_step_sim_launch_slotted_n(void* engine, uint32_t n_ticks, uint32_t n_win, uint32_t n_ranks,
                                    const uint32_t* rank_bounds, void* d_out, uint64_t slot_cap, void* routed_event);
/* tgsim_deliver_slotted_async of a fused group's exchange output (n_ranks x n_win chunks, source-rank
 * major): the windows' deliveries are appended in window order. */
int tgsim_deliver_slotted_n_async(void* engine, const void* d_in, uint32_t n_ranks, uint32_t n_win, uint64_t slot_cap,
                                  void* wait_event);
/* Phase 2: sorts the records addressed to this shard (DEVICE memory, n records) into the
 * delivery order and appends them to the drain buffer. */
int tgsim_deliver(void* engine, const void* d_in, size_t n);
/* Asynchronous phase 2: enqueues the delivery on the engine's delivery stream and returns.  The
 * stream first waits for wait_event (a hipEvent_t recorded after the producer of d_in, e.g. the
 * all-to-all; may be null), so the delivery of one step overlaps the next step's simulation.  d_in
 * must stay valid until tgsim_sync (or any reader) returns; no count check. */
int tgsim_deliver_async(void* engine, const void* d_in, size_t n, void* wait_event);
/* tgsim_deliver_async of a slotted exchange's output: n_ranks chunks of (slot_cap + 1) records,
 * each a count header and the records (the layout tgsim_step_sim_launch_slotted writes). */
int tgsim_deliver_slotted_async(void* engine, const void* d_in, uint32_t n_ranks, uint64_t slot_cap, void* wait_event);
/* Makes the engine's simulate stream wait for a hipEvent_t of another stream (e.g. the collective
 * that still reads the d_out buffer the next tgsim_step_sim will overwrite). */
int tgsim_wait_event(void* engine, void* event);
/* Records a hipEvent_t on the engine's delivery stream after every delivery enqueued so far (a
 * stream about to overwrite a delivery's input buffer waits for it). */
int tgsim_delivery_event(void* engine, void* event);
/* Waits for all of the engine's device work; reports a pending -EOVERFLOW. */
int tgsim_sync(void* engine);
/* Upper bound of records phase 1 can emit for the next step (for sizing d_out). */
int64_t tgsim_sim_capacity(void* engine);

/* Copies up to cap delivered records (oldest step first) and removes them; returns the count. */
int64_t tgsim_drain(void* engine, tgsim_delivery* out, size_t cap);
int64_t tgsim_pending_deliveries(void* engine);
/* Per-packet verdict bytes of the last step, in submit order (host packets) or generation order. */
int64_t tgsim_verdicts(void* engine, uint8_t* out, size_t cap);
int tgsim_stats(void* engine, tgsim_stats_t* out);

/* ---- RCCL exchange owned by the engine ---------------------------------- */
/* Replaces the cross-host delivery of the reference (weave CNI between k8s nodes,
 * pkg/sidecar/k8s_network.go:266-314): peers are partitioned over one engine per GPU (one process
 * per GPU), and scheduled records reach their destination's engine over RCCL (xGMI).  The engine
 * owns the communicator, its exchange stream and every buffer; a host only calls these functions
 * (INTEGRATION.md shows the Go loop).  librccl.so.1 is loaded on first use. */
#define TGSIM_COMM_ID_BYTES 128
/* A fresh communicator id (ncclGetUniqueId, 128 bytes into out_id).  One rank creates it and the
 * host hands it to every rank (the Go runner: through the sync service). */
int tgsim_comm_id(void* out_id);
/* Joins `engine` to the run's exchange as `rank` of `nranks` (<= 8) engines, one per GPU.  The
 * shards (tgsim_opts shard_begin/shard_end) must be contiguous in rank order and cover every peer;
 * they are gathered here.  Collective: every rank calls it with the same id. */
int tgsim_comm_init(void* engine, const void* id, int rank, int nranks);
/* One window on every rank (collective): simulate the owned sources, route the scheduled records
 * by destination shard, exchange the per-rank counts and then the records (grouped send/recv; the
 * own shard's records never leave the GPU), deliver them beside the next window's simulation.  The
 * host waits for this window's routing (one pinned-word poll) and for the count exchange: the
 * closed-loop form (gossip forwards, epoch reshaping) of tgsim_step. */
int tgsim_comm_step(void* engine, uint32_t n_ticks);
/* tgsim_comm_step in two halves: _launch enqueues the window's simulation and routing and returns,
 * so the host can stage the next window's ConfigureNetwork calls (they take effect at the next
 * launch) while the window simulates; _finish exchanges and delivers it. */
int tgsim_comm_launch(void* engine, uint32_t n_ticks);
int tgsim_comm_finish(void* engine);
/* n_steps pre-generated windows (tgsim_gen_storm) with the simulation two launches ahead of the
 * exchange, in groups of up to `fuse` (<= 8) windows per launch and per exchange, each rank's
 * records in fixed chunks of slot_cap records behind a count header (0: the largest per-rank count
 * of the earlier tgsim_comm_step windows, max over ranks, x 1.25 + 4096; without such windows the
 * bound of what one window can emit).  The host never waits for
 * the device.  A chunk that would overflow fails the run with -ENOSPC (nothing is lost silently).
 * Engines created with TGSIM_OPT_METRICS, or with the group matrix armed, run every window unfused
 * (their folds follow each window's kernel).  At one rank, and in tgsim_step_n, that happens by
 * itself; at two or more ranks every rank must agree on the group size, so fuse >= 2 (with n_steps >= 2)
 * is refused there with -EINVAL and that reason, on every rank, before a window is simulated (the clock does not
 * move, the generated windows stay queued): call it with fuse = 1. */
int tgsim_comm_run(void* engine, uint32_t n_ticks, uint32_t n_steps, uint32_t fuse, uint64_t slot_cap);
/* SignalAndWait over the shards (sync-service Barrier, sidecar_handler.go:40-44): the counts of
 * `state` are summed over the ranks by an all-reduce of the device counter tables; returns 1 when
 * the sum >= target, else 0.  Collective. */
int tgsim_comm_barrier(void* engine, uint32_t state, uint64_t target);
/* Every host wait of tgsim_comm_{step,finish,run,barrier} on a peer rank is bounded by
 * TGSIM_COMM_TIMEOUT_MS (read at tgsim_comm_init; default 300000): a rank whose peer stopped gets
 * -ETIMEDOUT naming the window, and every later tgsim_comm_* call on that engine fails the same way;
 * tgsim_destroy then aborts the communicator (ncclCommAbort) instead of waiting on it; with an RCCL
 * that has no ncclCommAbort it leaves the communicator, its stream and buffers allocated (a message on
 * stderr) rather than wait forever. */
typedef struct {
    int32_t rank, nranks;
    uint64_t exchanged_records; /* records (slotted: record slots) this rank has sent, self included */
    uint64_t max_rank_count;    /* largest per-rank count a tgsim_comm_step window routed here */
    uint64_t slot_cap;          /* chunk capacity of the last tgsim_comm_run                    */
    uint32_t bounds[9];         /* rank r owns peers [bounds[r], bounds[r + 1])                 */
    uint32_t _pad;
} tgsim_comm_info_t;
int tgsim_comm_info(void* engine, tgsim_comm_info_t* out);

/* ---- gossip workload (C4) ------------------------------------------------------------------ */
/* Arms the gossip driver (-EBUSY while the ping or flow driver is armed): resets the per-peer receipt
 * state of this shard and schedules the floods whose origin it owns.  Requires lookahead_ns >= the
 * window of every later step and <= the minimum netem delay, so that a window's receipts are known
 * before the next window. */
int tgsim_gossip_init(void* engine, const tgsim_gossip* g);
/* Generates the next n_ticks window of gossip traffic on the device (origins + forwards of the
 * receipts delivered so far), like tgsim_gen_storm.  The generation runs ahead of the host, so a
 * receipt that precedes the window (lookahead shorter than the window) is reported with -EINVAL by
 * the step that consumes it (or tgsim_sim_capacity, or the next tgsim_gen_gossip): that window and
 * every window queued after it are dropped without changing any peer's forwarded floods, and the
 * error stays until tgsim_gossip_init. */
int tgsim_gen_gossip(void* engine, uint32_t n_ticks);
/* Per flood, the number of this shard's peers that have the flood (received or originated);
 * out[0..n_floods).  Returns n_floods. */
int64_t tgsim_gossip_reached(void* engine, uint64_t* out, size_t cap);

/* Propagation of flood f over this shard's peers.  hold(s, f) = the tick at which peer s offers its
 * forwards of flood f, minus the flood's start tick (start_tick + f * start_gap_ticks): 0 for the
 * origin, floor(d / tick) + 1 - start for a peer whose earliest uncorrupted receipt was delivered at
 * d.  Only peers that have forwarded the flood count (the same set tgsim_gossip_reached counts): a
 * receipt still pending for a later window is not in the report. */
typedef struct {
    uint64_t reached;    /* peers of this shard that have forwarded the flood          */
    uint64_t sum_ticks;  /* sum of hold over them                                      */
    uint32_t min_ticks;  /* 0xFFFFFFFF when reached == 0                               */
    uint32_t max_ticks;  /* 0 when reached == 0                                        */
} tgsim_gossip_flood;    /* 24 B */

/* Reduced on the device; no per-peer table crosses to the host.  floods[0 .. min(cap, n_floods)) and,
 * when n_bins > 0, hist[f * n_bins + b] = peers with min(hold / bin_ticks, n_bins - 1) == b (the last
 * bin collects everything beyond).  n_bins 0 (hist may be NULL) .. 256; bin_ticks >= 1 when
 * n_bins > 0.  Returns n_floods.  Synchronizes like tgsim_gossip_reached.  Per-shard results merge
 * by sum / sum / min / max / sum.  -EINVAL (with a tgsim_last_error text) when the gossip driver is
 * not armed, n_bins > 256, bin_ticks == 0 or hist == NULL with n_bins > 0, floods == NULL with
 * cap > 0.  A late receipt (tgsim_gen_gossip) does not block the report. */
int64_t tgsim_gossip_spread(void* engine, uint32_t bin_ticks, uint32_t n_bins,
                            tgsim_gossip_flood* floods, uint64_t* hist, size_t cap);

/* The forward ticks themselves (absolute) for peers [peer, peer + n) of this shard, row-major
 * [n][n_floods], 0xFFFFFFFF where the peer has not forwarded the flood; compacted and masked on the
 * device.  Returns the words written, -EINVAL for a range outside the shard, -ENOSPC when
 * cap < n * n_floods. */
int64_t tgsim_gossip_times(void* engine, uint32_t peer, uint32_t n, uint32_t* out, size_t cap);

/* ---- ping mesh (C1/C2 and plans/verify as one closed loop on the device) -------------------- */
/* Every peer probes the targets in its slots on a fixed schedule; echo replies are generated on the
 * device from each window's delivered records, wait in a device calendar for the window that holds
 * their tick, and loss and round-trip time are folded per (peer, slot) pair as replies are
 * delivered.  No delivery has to reach the host.
 *
 *   Request  peer s, slot k, probe j: one packet s -> targets[s * fanout + k], seq = j * fanout + k,
 *            `len` bytes, at tick start_tick + j * interval_ticks.  A target is a peer id other
 *            than s, TGSIM_EXTERNAL, or TGSIM_PING_NONE (an empty slot sends nothing and is not a
 *            pair).
 *   Reply    a delivered request record with neither TGSIM_FLAG_DUP nor TGSIM_FLAG_CORRUPT,
 *            addressed to r, from q, delivered at d, makes r offer one packet r -> q, seq =
 *            0x80000000 | request seq, `len` bytes, at tick floor(d / tick_ns) + 1.  Clones and
 *            corrupted copies are ignored and counted (dup_ignored first, else corrupt_ignored).  A
 *            non-clone record exists at most once per offered packet, so a probe has at most one
 *            counted reply.
 *   Receipt  a delivered reply with neither flag, at d, credits the pair (dst, k = (seq &
 *            0x7FFFFFFF) % fanout) with rtt_ns = d - (start_tick + j * interval_ticks) * tick_ns,
 *            j = (seq & 0x7FFFFFFF) / fanout.  Records count when a step emits them (when
 *            tgsim_drain would show them).  A record that matches no probe of the schedule (traffic
 *            queued before the driver was armed) is neither answered nor credited.
 *   Order    within one source's window the offered packets are ordered by (tick, seq, dst).
 *   Loop     as for gossip, every later window <= lookahead_ns <= the minimum netem delay.  A
 *            calendar entry whose tick precedes the window being generated is a late receipt:
 *            tgsim_gen_ping fails with -EINVAL (tgsim_last_error names the tick), nothing is
 *            generated, and the error stays until the next tgsim_ping_init; the reports stay
 *            readable.
 * tgsim_ping_init arms a single engine that owns every peer; tgsim_ping_init_sharded (below) arms one
 * engine per shard of a run spread over tgsim_comm_*: replies are generated at the destination's
 * shard from the records it receives, so the sharded form needs no exchange of its own. */
#define TGSIM_PING_NONE 0xFFFFFFFEu      /* targets[] entry: empty slot */
typedef struct {
    uint32_t fanout;         /* target slots per peer, 1..64                              */
    uint32_t count;          /* probes per slot, 1..65535                                 */
    uint32_t interval_ticks; /* >= 1; probe j of every slot is offered at start + j*interval */
    uint32_t len;            /* bytes on the wire, 1..65535, request and reply            */
    uint64_t start_tick;     /* absolute tick of probe 0, >= the engine's next window     */
    uint64_t bin_ns;         /* RTT histogram bin width, >= 1 when n_bins > 0             */
    uint32_t n_bins;         /* 0..256; the last bin collects everything beyond           */
    uint32_t _pad;
} tgsim_ping;                /* 40 B */
typedef struct {             /* one (peer, slot); 32 B */
    uint32_t sent;           /* probes of this slot offered so far (start + j*interval < now_tick) */
    uint32_t received;       /* counted replies                                            */
    uint64_t sum_ns, min_ns /* UINT64_MAX when none */, max_ns /* 0 when none */;
} tgsim_ping_pair;
typedef struct {
    uint64_t pairs, sent, received, sum_ns, min_ns, max_ns;
    uint64_t pairs_all;       /* sent > 0 and received == sent  */
    uint64_t pairs_none;      /* sent > 0 and received == 0     */
    uint64_t dup_ignored, corrupt_ignored; /* records skipped on either leg                */
    uint64_t pending_replies; /* replies recorded but not yet offered (the calendar)       */
} tgsim_ping_summary;
/* Arms the driver (targets: [n_peers][fanout]).  -EINVAL (with a tgsim_last_error text) for an
 * engine that does not own every peer, a bad field, a target that is the peer itself or out of range
 * (the text names the entry), or a start tick in the past; -EBUSY while the gossip or flow driver is armed
 * or while host packets or generated windows are pending.  While armed, tgsim_submit,
 * tgsim_gen_storm, tgsim_gossip_init and the tgsim_step_sim* / tgsim_comm_* steps return -EBUSY and
 * tgsim_step_n runs its windows one by one.  tgsim_configure between windows is allowed: a purged or
 * disconnected leg simply never produces a receipt.  tgsim_ping_init(engine, NULL, NULL) disarms and
 * frees the state (a no-op when the ping driver is not armed, an armed flow driver included). */
int tgsim_ping_init(void* engine, const tgsim_ping* p, const uint32_t* targets);
/* Generates the next n_ticks window on the device, like tgsim_gen_storm: the scheduled probes and the
 * calendar's replies due in it; the entries not yet due stay in the calendar.  One window at a time
 * (-EBUSY while a generated window is pending). */
int tgsim_gen_ping(void* engine, uint32_t n_ticks);
/* The summary over every pair, reduced on the device, and (n_bins > 0) hist[b] = counted replies
 * with min(rtt_ns / bin_ns, n_bins - 1) == b; hist_cap >= n_bins.  Returns n_bins. */
int64_t tgsim_ping_report(void* engine, tgsim_ping_summary* out, uint64_t* hist, size_t hist_cap);
/* The pair rows of peers [peer, peer + n), row-major [n][fanout] (an empty slot: sent 0, received 0);
 * returns the rows written, -ENOSPC when cap < n * fanout. */
int64_t tgsim_ping_pairs(void* engine, uint32_t peer, uint32_t n, tgsim_ping_pair* out, size_t cap);

/* ---- ping mesh over shards ------------------------------------------------------------------ */
/* Arms the ping driver on an engine that owns peers [shard_begin, shard_end), which may be every
 * peer.  `targets` is the WHOLE run's table [n_peers][fanout], the same on every shard: it is
 * replicated like the peer tables, because a responder's shard validates a request against the
 * requester's row, which it does not own (4 B x fanout per peer and shard: 32 MB at 1M peers with
 * fanout 8).  Every field rule, -EINVAL text and -EBUSY rule of tgsim_ping_init holds, less the
 * ownership test.  (engine, NULL, NULL) disarms, frees the state and drops a generated window of its
 * own that is still pending (the window of a step the ranks refused, see the late rule);
 * tgsim_ping_init(engine, NULL, NULL) disarms either form.
 *
 * Request, reply, receipt, order and loop are exactly those above.  What differs is where things
 * happen:
 *   Requests of peer s are generated by the shard that owns s (tgsim_gen_ping generates the owned
 *            sources' rows and involves no collective).
 *   Calendar an entry is made from a delivered request addressed to r at the shard that owns r, where
 *            the exchange's delivery emits the record; it becomes r's reply there.
 *   Receipt  a delivered reply addressed to q credits pair (q, k) at q's shard: each shard holds the
 *            pair rows of its own peers only.
 *   Counters dup_ignored and corrupt_ignored count at the shard that emits the record;
 *            pending_replies is that shard's calendar.
 * While armed through this call the closed steps are accepted: tgsim_comm_step, tgsim_comm_launch /
 * tgsim_comm_finish and, underneath them, tgsim_step_sim, tgsim_step_sim_launch / _finish / _counts,
 * tgsim_deliver / tgsim_deliver_async and tgsim_deliver_slotted_async with one window; tgsim_step on
 * an engine that owns every peer gives the results of the unsharded form.  tgsim_comm_run,
 * tgsim_step_sim_launch_slotted called directly and tgsim_step_sim_launch_slotted_n stay -EBUSY
 * (pipelined or fused: they cannot be closed-loop), as do tgsim_submit, tgsim_gen_storm,
 * tgsim_gossip_init and tgsim_flow_init; one generated window at a time, and none between
 * tgsim_comm_launch and its tgsim_comm_finish (-EBUSY: the window's receipts come first).
 *
 * tgsim_ping_report gives THIS shard's summary and histogram.  Reports merge over the shards field by
 * field: every field by sum, except min_ns by min and max_ns by max; hist by sum, bin by bin (a shard
 * without a reply reports the neutral min_ns UINT64_MAX and max_ns 0).  tgsim_comm_ping_report does
 * that on the device.  tgsim_ping_pairs takes global peer ids inside the shard (-EINVAL, naming both
 * ranges, otherwise).
 *
 * The late rule across ranks.  A late receipt is seen by ONE rank's tgsim_gen_ping: it returns
 * -EINVAL, generates nothing and changes no state, and the error stays, as above.  Host protocol:
 * every rank calls tgsim_comm_step / tgsim_comm_launch for every window, even after its own
 * generation failed.  With more than one rank the launch first agrees on the ranks' fault flags (one
 * 8-byte max all-reduce on the exchange stream and one host wait per window); when any rank is late,
 * EVERY rank's call returns -EINVAL, tgsim_last_error names the late rank and the tick, nothing is
 * simulated, and the error stays on every rank until it re-arms (later calls fail at once, without a
 * collective).  The reports stay readable.  A calendar overflow (-ENOSPC) is agreed the same way.
 * With one rank nothing is exchanged for this. */
int tgsim_ping_init_sharded(void* engine, const tgsim_ping* p, const uint32_t* targets);
/* The WHOLE run's summary and histogram on every rank (collective, after tgsim_comm_init): each
 * rank's local report is packed on the device into three runs (sums and histogram bins, min_ns,
 * max_ns), reduced by three u64 all-reduces (sum, min, max) on the exchange stream and unpacked;
 * no per-pair table crosses between GPUs or to the host.  Returns n_bins; -EINVAL without a
 * communicator or when the driver is not armed through tgsim_ping_init_sharded, -ETIMEDOUT as the
 * other collectives.  With one rank it equals tgsim_ping_report. */
int64_t tgsim_comm_ping_report(void* engine, tgsim_ping_summary* out, uint64_t* hist, size_t hist_cap);

/* ---- reliable transfers (windowed flows, per-segment ACKs and retransmission timers) --------- */
/* "Send n_seg segments reliably from a to b" as a closed loop on the device: how
 * long a transfer takes and what goodput it reaches on links with this latency, loss, bandwidth and
 * netem queue limit.  It is NOT TCP: no handshake, no congestion control (unless
 * armed with tgsim_flow_init_cc, further down), no cumulative ACK.  A fixed
 * window, a selective ACK per delivered segment, a retransmission timer per segment: the smallest
 * protocol that completes under loss, saturates a link whose bandwidth-delay product the window
 * covers, and is a pure function of the delivered records.
 *
 *   Table    flow f = {src, dst, n_seg, start_tick}, sorted by src (non-decreasing): a source's flows
 *            are contiguous and a flow's slot is its rank among them, at most TGSIM_FLOW_SLOTS per
 *            source.  dst is a peer other than src (not TGSIM_EXTERNAL), 1 <= n_seg <= 2^23,
 *            start_tick >= the engine's next window; every tick the schedule can reach is < 2^31.
 *   Seq      bit 31 ACK | bits 27..30 attempt | bits 23..26 slot | bits 0..22 segment.  The attempt is
 *            in the key on purpose: Philox is keyed by (seed, src, dst, seq), so a retransmission
 *            draws afresh.
 *   Sender   per flow: base (lowest unacknowledged segment), next (lowest segment never released;
 *            always min(base + window, n_seg)), an acked bitmap over [base, base + 64), per in-flight
 *            segment a due tick and an attempt count, counters, done_ns.  At arming base = 0 and the
 *            segments [0, min(window, n_seg)) are due at start_tick with attempt 0.
 *   Offer    generating the window [T, T + n): every unacknowledged in-flight segment i of a live flow
 *            with T <= due_i < T + n is offered as one packet src -> dst of seg_len bytes at tick
 *            due_i, seq = attempt_i << 27 | slot << 23 | i; then due_i += rto_ticks, attempt_i += 1.
 *            A segment that becomes due with attempt_i == max_attempts fails the flow: with F the
 *            earliest such due tick of the flow in the window, segments due before F are still
 *            offered, nothing is offered at or after F, and the flow is FAILED with fail_tick = F (by
 *            tick, not by window: the result does not depend on the step length).  n > rto_ticks is
 *            -EINVAL: a segment is offered at most once per window.
 *   ACK      the receiver is stateless.  A delivered data record with neither TGSIM_FLAG_DUP nor
 *            TGSIM_FLAG_CORRUPT, addressed to r, from q, whose slot is below q's flow count, whose
 *            flow's dst == r and whose segment is < n_seg, makes r offer one packet r -> q of ack_len
 *            bytes, seq = 0x80000000 | data seq, at tick floor(d / tick_ns) + 1 (d: the delivery time;
 *            the ping reply rule).  Every delivered attempt is acknowledged.  Clones and corrupted
 *            copies are ignored and counted on either leg (dup_ignored first, else corrupt_ignored).
 *   Receipt  a flow's ACKs take effect in delivery order, (t_ns, src, seq) within the sender's
 *            records.  An unflagged ACK delivered at d matches flow (its dst, its slot) when the slot
 *            is valid, the flow's dst equals the ACK's src and the segment is < n_seg.  A matching
 *            ACK is stale (counted in stale_acks, nothing else) when the flow is DONE or FAILED, or
 *            seg < base, or seg >= next, or the segment is already acknowledged.  Otherwise the
 *            segment is marked acknowledged; base advances over the acknowledged prefix; every
 *            segment that enters [base, base + window) and is < n_seg is released with due =
 *            floor(d / tick_ns) + 1, attempt 0; when base == n_seg the flow is DONE with done_ns = d.
 *            Flow completion time (FCT) = done_ns - start_tick * tick_ns.  Records count when a step
 *            emits them (when tgsim_drain would show them); traffic that matches no flow is neither
 *            acknowledged nor credited.
 *   Order    within one source's window the offered packets are ordered by (tick, seq, dst).
 *   Loop     as for ping, every later window <= lookahead_ns <= the minimum netem delay.  A calendar
 *            ACK, or a released segment, whose tick precedes the window being generated is a late
 *            receipt: tgsim_gen_flow fails with -EINVAL (tgsim_last_error names the tick), nothing is
 *            generated, no flow state changes, and the error stays until the next tgsim_flow_init;
 *            the reports stay readable.
 *   Verdicts the sender learns nothing from them: a filtered, lost or queue-full segment is recovered
 *            by its timer only (unless armed with tgsim_flow_init_fb, further down: the verdict
 *            feedback counts them per flow and can fail a flow on a refusal).
 * tgsim_flow_init and its _cc / _rto / _fb forms arm a single engine that owns every peer;
 * tgsim_flow_init_sharded (further down) arms one engine per shard of a run spread over tgsim_comm_*. */
#define TGSIM_FLOW_SLOTS 16u
enum tgsim_flow_state { TGSIM_FLOW_ACTIVE = 0, TGSIM_FLOW_DONE = 1, TGSIM_FLOW_FAILED = 2 };
typedef struct {
    uint32_t seg_len;      /* bytes on the wire of a data segment, 1..65535            */
    uint32_t ack_len;      /* bytes on the wire of an ACK, 1..65535                    */
    uint32_t window;       /* segments in flight, 1..64                                */
    uint32_t rto_ticks;    /* retransmission timer, >= 1                               */
    uint32_t max_attempts; /* offers per segment before the flow fails, 1..16          */
    uint32_t n_bins;       /* FCT histogram, 0..256; the last bin collects everything beyond */
    uint64_t bin_ns;       /* >= 1 when n_bins > 0                                     */
} tgsim_flow;              /* 32 B */
typedef struct {
    uint32_t src, dst, n_seg, start_tick;
} tgsim_flow_spec;         /* 16 B */
typedef struct {           /* one flow; 32 B */
    uint32_t state;        /* enum tgsim_flow_state                                    */
    uint32_t acked;        /* segments acknowledged                                    */
    uint32_t offered;      /* data packets offered                                     */
    uint32_t retransmits;  /* of them, offers with attempt > 0                         */
    uint32_t stale_acks;
    uint32_t base;
    uint64_t done_ns;      /* DONE: delivery time of the last ACK; FAILED: fail_tick * tick_ns; ACTIVE: 0 */
} tgsim_flow_row;
typedef struct {
    uint64_t flows, done, failed, active;
    uint64_t segs_acked, bytes_acked; /* bytes_acked = segs_acked * seg_len                    */
    uint64_t data_offered, retransmits, stale_acks;
    uint64_t dup_ignored, corrupt_ignored; /* records skipped on either leg                    */
    uint64_t pending_acks;            /* ACKs recorded but not yet offered (the calendar)      */
    uint64_t fct_sum_ns, fct_min_ns /* UINT64_MAX when none */, fct_max_ns; /* over DONE flows */
} tgsim_flow_summary;      /* 120 B */
/* Arms the driver.  -EINVAL (with a tgsim_last_error text that names the entry) for an engine that
 * does not own every peer, a bad field, an unsorted table, a 17th flow of a source, dst == src or out
 * of range, or a start tick in the past; -EBUSY while the gossip or ping driver is armed or while host
 * packets, generated windows or launched steps are pending.  While armed, tgsim_submit,
 * tgsim_gen_storm, tgsim_gossip_init, tgsim_ping_init and the tgsim_step_sim* / tgsim_comm_* steps
 * return -EBUSY, tgsim_step_n runs its windows one by one, and one generated window may be pending.
 * tgsim_configure between windows is allowed; that is the point: reshape or partition a link
 * mid-transfer.  tgsim_flow_init(engine, NULL, NULL, 0) disarms and frees the state. */
int tgsim_flow_init(void* engine, const tgsim_flow* p, const tgsim_flow_spec* flows, uint64_t n_flows);
/* Generates the next n_ticks window on the device, like tgsim_gen_ping: the segments due in it and the
 * calendar's ACKs due in it.  One window at a time (-EBUSY while a generated window is pending). */
int tgsim_gen_flow(void* engine, uint32_t n_ticks);
/* The summary over every flow, reduced on the device, and (n_bins > 0) hist[b] = DONE flows with
 * min(fct / bin_ns, n_bins - 1) == b; hist_cap >= n_bins.  Returns n_bins.  Synchronizes, and fails,
 * like tgsim_ping_report. */
int64_t tgsim_flow_report(void* engine, tgsim_flow_summary* out, uint64_t* hist, size_t hist_cap);
/* The rows of flows [first, first + n) of the table; returns the rows written, -EINVAL for a range
 * outside the table, -ENOSPC when cap < n (as tgsim_ping_pairs). */
int64_t tgsim_flow_rows(void* engine, uint64_t first, uint64_t n, tgsim_flow_row* out, size_t cap);

/* ---- congestion control of the flow driver (opt-in per arming) --------------- */
/* An AIMD congestion window and a fast retransmit on top of the rules above: how transfers back off
 * and share a shaped link, what goodput survives loss, what happens when one instance's connections
 * overrun the netem queue.  Armed with tgsim_flow_init_cc and a non-NULL cc; without it every rule
 * above holds as written.  With it, `window` is the cap of the congestion window (the receiver
 * window), and everything above that is not named here stays as written: the seq layout, the ACK
 * leg, the stale rule, the fail rule by tick, the order, the loop and late rule, and verdicts
 * teaching the sender nothing.
 *
 *   State     per flow, beside the row: cwnd (1..window), ssthresh (2..max(window, 2)), cwnd_cnt, next
 *             (lowest segment never released; now stored), recover, and the counters loss_events,
 *             fast_retransmits, timeouts: the 32-B tgsim_flow_cc_row.  Per in-flight segment a FAST
 *             flag beside its attempt count.
 *   Invariant base <= next <= min(base + window, n_seg): the timers' ring (segment mod window) and the
 *             64-bit bitmap hold as before.
 *   Arming    cwnd = init_cwnd, ssthresh = init_ssthresh ? init_ssthresh : window, next =
 *             min(init_cwnd, n_seg), recover = 0, cwnd_cnt = 0; the segments [0, next) are due at
 *             start_tick with attempt 0.
 *   In flight [base, next), wherever the rules above say [base, min(base + window, n_seg)): the offer
 *             pass, the late test and the stale test (seg >= next).
 *   Receipt   of a non-stale ACK of seg delivered at d, tick = floor(d / tick_ns) + 1, in this order:
 *             1. the segment is marked acknowledged, acked += 1;
 *             2. base advances over the acknowledged prefix;
 *             3. growth, only when base >= recover: cwnd += 1 when cwnd < ssthresh; otherwise
 *                cwnd_cnt += 1, and when cwnd_cnt >= cwnd then cwnd += 1 and cwnd_cnt = 0; then cwnd =
 *                min(cwnd, window);
 *             4. fast retransmit, when dupthresh > 0: every unacknowledged segment i of [base, next),
 *                in ascending order, with at least dupthresh acknowledged segments above it, an attempt
 *                count of exactly 1, no FAST flag and a due tick > tick, gets due = tick and the FAST
 *                flag, fast_retransmits += 1; when i >= recover that is a loss event: ssthresh =
 *                max(cwnd / 2, 2), cwnd = ssthresh, cwnd_cnt = 0, recover = next, loss_events += 1;
 *             5. release: next2 = max(next, min(base + cwnd, n_seg)); the segments [next, next2) get
 *                due = tick, attempt 0, no flag; next = next2;
 *             6. base == n_seg makes the flow DONE, as above.
 *   Offer     as above.  The retransmission of a FAST segment carries attempt 1 in its seq; its timer
 *             restarts at its tick + rto_ticks, its attempt count becomes 2 and the flag clears.  An
 *             offer with attempt k > 0 and no FAST flag is a timeout, timeouts += 1.  When a timeout of
 *             this generation has seg >= recover (recover as it was before the generation, so the order
 *             the segments are walked in does not matter), that is one loss event of the flow in this
 *             generation: ssthresh = max(cwnd / 2, 2), cwnd = 1, cwnd_cnt = 0, recover = next,
 *             loss_events += 1.  A late window still changes no state, the cc rows included.  A
 *             FAST segment is due like any other: with max_attempts == 1 it fails the flow at its tick.
 *   Step      as above, the counters and the windows depend on the step length, the fail tick does not.
 *   Not here  cumulative or delayed ACKs and pacing; an RTT estimator and timer backoff
 *             (tgsim_flow_init_rto) and failing at once on a refusal verdict (tgsim_flow_init_fb)
 *             are opt-in further down. */
typedef struct {
    uint32_t init_cwnd;     /* 1..window: segments released at start_tick                  */
    uint32_t init_ssthresh; /* 0 -> window; else 2..window                                  */
    uint32_t dupthresh;     /* 0: timer only; 1..63: fast retransmit after this many        */
                            /* acknowledged segments above a hole                           */
    uint32_t _pad;
} tgsim_flow_cc;            /* 16 B */
typedef struct {            /* one flow; 32 B */
    uint32_t cwnd, ssthresh, next, recover, cwnd_cnt;
    uint32_t loss_events, fast_retransmits, timeouts;
} tgsim_flow_cc_row;
typedef struct {            /* 64 B */
    uint64_t loss_events, fast_retransmits, timeouts;
    uint64_t active, cwnd_sum, cwnd_min /* UINT64_MAX when none */, cwnd_max; /* over ACTIVE flows */
    uint64_t _pad;
} tgsim_flow_cc_summary;
/* tgsim_flow_init with congestion control: every arming, busy and disarm rule of tgsim_flow_init
 * holds, cc == NULL is tgsim_flow_init itself, and a bad cc field is -EINVAL with a tgsim_last_error
 * text that names the field and its value. */
int tgsim_flow_init_cc(void* engine, const tgsim_flow* p, const tgsim_flow_cc* cc,
                       const tgsim_flow_spec* flows, uint64_t n_flows);
/* The cc rows of flows [first, first + n), and the cc summary reduced on the device.  -EINVAL
 * ("congestion control is not armed") when flows are armed without cc or not at all; otherwise they
 * synchronize, and fail, like tgsim_flow_rows and tgsim_flow_report. */
int64_t tgsim_flow_cc_rows(void* engine, uint64_t first, uint64_t n, tgsim_flow_cc_row* out, size_t cap);
int     tgsim_flow_cc_report(void* engine, tgsim_flow_cc_summary* out);

/* ---- RTT estimator and timer backoff of the flow driver (opt-in per arming) -- */
/* A retransmission timer per flow that follows the flow's measured round trip (RFC 6298 in integer
 * ticks) and, optionally, doubles per earlier offer of a segment: what a run over links of unequal
 * latency needs, where no one rto_ticks is right.  Armed with tgsim_flow_init_rto and a non-NULL rto,
 * with or without cc (the two are independent); without it every rule above holds as written.  With
 * it, everything above that is not named here stays as written.
 *
 *   State     per flow, the 32-B tgsim_flow_rto_row: srtt8 (smoothed RTT x 8), rttvar4 (variation x 4),
 *             rto (the flow's current timer), samples, rtt_min, rtt_max, rtt_last, all in ticks.  Per
 *             in-flight segment a `sent` tick beside its due tick and attempt count, on the same ring
 *             (segment mod window).
 *   Arming    rto = p->rto_ticks (the initial timer), srtt8 = rttvar4 = samples = rtt_max = rtt_last =
 *             0, rtt_min = 0xFFFFFFFF.
 *   Offer     a segment offered at tick t with attempt count k before the offer: its timer restarts at
 *             t + timer, timer = backoff ? min((uint64)rto << k, max_rto_ticks) : rto, with rto the
 *             flow's value as the generation finds it (a generation changes no rto row, so the order
 *             the segments are walked in does not matter).  k counts every earlier offer of the
 *             segment, a fast retransmission included.  When k == 0, sent = t.  The fail rule stays by
 *             tick and by max_attempts: with backoff a flow that never gets an ACK fails at start_tick
 *             + the sum over k < max_attempts of min(rto << k, max_rto_ticks).
 *   Sample    a non-stale ACK whose attempt field (seq bits 27..30) is 0 and whose segment has been
 *             offered (attempt count >= 1), delivered at d, tick = floor(d / tick_ns) + 1, gives m =
 *             min(tick - sent, max_rto_ticks).  The ACK echoes the attempt it answers, so the sample
 *             is unambiguous however often the segment was retransmitted since: no Karn exclusion, and
 *             a flow whose initial timer is below its round trip still gets its first sample.
 *   Update    before anything else uses the ACK (ahead of step 1 of the cc receipt).  First sample:
 *             srtt8 = 8 m, rttvar4 = 2 m.  Later: err = m - (srtt8 >> 3), signed; rttvar4 = rttvar4 -
 *             (rttvar4 >> 2) + |err|; srtt8 += err.  Then rto = clamp((srtt8 >> 3) + max(rttvar4, 1),
 *             min_rto_ticks, max_rto_ticks); samples += 1; rtt_min, rtt_max and rtt_last follow m.
 *             max_rto_ticks <= 2^27 keeps every field inside 32 bits.
 *   Window    while armed with rto, tgsim_gen_flow(n) is -EINVAL when n > min_rto_ticks (the text names
 *             min_rto_ticks), in place of the rto_ticks test: a segment is still offered at most once
 *             per window.
 *   Late      a late window changes no state, the rto rows and `sent` included.
 *   Step      as above, the counters and the samples depend on the step length, the fail tick does not.
 *   Not here  cumulative or delayed ACKs and pacing; failing at once on a refusal verdict is opt-in
 *             further down (tgsim_flow_init_fb). */
typedef struct {
    uint32_t min_rto_ticks; /* >= 1; also the longest window tgsim_gen_flow accepts while armed */
    uint32_t max_rto_ticks; /* min_rto_ticks .. 2^27                                            */
    uint32_t backoff;       /* 0: a segment's timer is the flow's rto; 1: doubled per earlier   */
                            /* offer of the segment                                             */
    uint32_t _pad;
} tgsim_flow_rto;           /* 16 B */
typedef struct {            /* one flow; 32 B */
    uint32_t srtt8;         /* smoothed RTT x 8, ticks; 0 with no sample                        */
    uint32_t rttvar4;       /* RTT variation x 4                                                */
    uint32_t rto;           /* the flow's current timer, ticks                                  */
    uint32_t samples;
    uint32_t rtt_min /* 0xFFFFFFFF when none */, rtt_max, rtt_last, _pad;
} tgsim_flow_rto_row;
typedef struct {            /* 64 B; every field but samples is over the flows with samples > 0 */
    uint64_t samples, sampled_flows;
    uint64_t srtt_sum, srtt_min /* UINT64_MAX when none */, srtt_max;   /* srtt8 >> 3 */
    uint64_t rto_sum, rto_min /* UINT64_MAX when none */, rto_max;
} tgsim_flow_rto_summary;
/* tgsim_flow_init_cc with the estimator: every arming, busy and disarm rule of tgsim_flow_init holds,
 * rto == NULL is tgsim_flow_init_cc itself, cc may be NULL or not, and a bad rto field is -EINVAL with
 * a tgsim_last_error text that names the field and its value: min_rto_ticks == 0, max_rto_ticks below
 * min_rto_ticks or above 2^27, backoff > 1, p->rto_ticks outside [min_rto_ticks, max_rto_ticks]. */
int tgsim_flow_init_rto(void* engine, const tgsim_flow* p, const tgsim_flow_cc* cc, const tgsim_flow_rto* rto,
                        const tgsim_flow_spec* flows, uint64_t n_flows);
/* The rto rows of flows [first, first + n), and the rto summary reduced on the device.  -EINVAL ("the
 * RTT estimator is not armed") when flows are armed without rto or not at all; otherwise they
 * synchronize, and fail, like tgsim_flow_cc_rows and tgsim_flow_cc_report. */
int64_t tgsim_flow_rto_rows(void* engine, uint64_t first, uint64_t n, tgsim_flow_rto_row* out, size_t cap);
int     tgsim_flow_rto_report(void* engine, tgsim_flow_rto_summary* out);

/* ---- verdict feedback of the flow driver (opt-in per arming) ---------------- */
/* What became of a flow's offers, and a sender that learns of a refusal as a real one does (EINVAL
 * or EACCES on the first write, see TGSIM_V_BLACKHOLE and TGSIM_V_PROHIBIT): per-flow verdict
 * counters folded on the device after each window's simulation, and a mask of refusal verdicts that
 * fail a flow at the tick of the refused offer.  Armed with tgsim_flow_init_fb and a non-NULL fb,
 * with or without cc and rto (the three are independent); without it every rule above holds as
 * written.  With it, everything above that is not named here stays as written.
 *
 *   State     per flow, the 32-B tgsim_flow_fb_row, all zero at arming.
 *   Fold      after the window [T, T + n) has been simulated, every data packet the driver offered in
 *             it (seq bit 31 clear) is attributed to its flow (its source, slot bits 23..26), and the
 *             low nibble v of its verdict byte is counted: 0 -> scheduled, 5 -> lost, 6 -> queue_full,
 *             1..4 -> refused; a high nibble other than TGSIM_V_NONE adds one to cloned.  Every flow
 *             is counted, whatever its state: after every step scheduled + lost + queue_full + refused
 *             == the flow row's offered.  ACK packets are attributed to no flow: their verdicts are
 *             tgsim_stats_t.by_verdict less these sums.
 *   Fail      the offer tick of a packet is T + its tick.  Let R be the flow's refused offers of this
 *             window whose verdict v has bit 1 << v set in fail_mask.  When R is not empty and the flow
 *             is ACTIVE, or was failed by this very window's generation (FAILED, fail_verdict == 0,
 *             done_ns >= T * tick_ns: the timer rule stopped its offers at a later tick of the same
 *             window), then with F the earliest offer tick in R: state = FAILED, done_ns = F *
 *             tick_ns, and fail_verdict, fail_seg and fail_attempt come from the offer of R at tick F
 *             with the lowest seq.  Offers of the flow later in that window were already made and stay
 *             counted in offered; their ACKs are stale.  FAILED is final.  A refused ACK fails
 *             nothing: the receiver stays stateless and the sender's timer handles it as before.
 *   Order     a window's verdicts take effect before the records the same step emits are folded: an
 *             ACK delivered in the step that failed its flow is stale.  The cc and rto rows of a flow
 *             failed by verdict stay as they were.
 *   Late      a late window is never simulated, so it changes no fb row.
 *   Step      the fail tick is by tick, like the timer's, and does not depend on the step length; the
 *             counters do.
 *   Not here  reacting to a local QUEUE_FULL as a congestion signal (it is counted only). */
/* bits a fail_mask may carry: 1<<TGSIM_V_DISCONNECTED | 1<<TGSIM_V_NO_ROUTE | 1<<TGSIM_V_BLACKHOLE | 1<<TGSIM_V_PROHIBIT */
#define TGSIM_FLOW_FB_REFUSALS 0x1Eu
typedef struct {
    uint32_t fail_mask;     /* bit 1 << v: a data offer refused with verdict v fails its flow; 0: count only */
    uint32_t _pad[3];
} tgsim_flow_fb;            /* 16 B */
typedef struct {            /* one flow; 32 B */
    uint32_t scheduled, lost, queue_full, refused; /* the flow's data offers by verdict, low nibble 0 / 5 / 6 / 1..4 */
    uint32_t cloned;        /* data offers whose high nibble is not TGSIM_V_NONE                         */
    uint32_t fail_verdict;  /* 0: not failed, or failed by its timer; else the refusing verdict 1..4      */
    uint32_t fail_seg, fail_attempt; /* segment and attempt field of the refused offer; 0 when fail_verdict == 0 */
} tgsim_flow_fb_row;
typedef struct {            /* 96 B */
    uint64_t scheduled, lost, queue_full, refused, cloned;
    uint64_t refused_flows; /* flows with refused > 0                                   */
    uint64_t failed_timer;  /* FAILED with fail_verdict == 0                            */
    uint64_t failed_by[4];  /* FAILED with fail_verdict == 1 + index                    */
    uint64_t _pad;
} tgsim_flow_fb_summary;
/* tgsim_flow_init_rto with the verdict feedback: every arming, busy and disarm rule of tgsim_flow_init
 * holds, fb == NULL is tgsim_flow_init_rto itself, cc and rto may each be NULL or not, and a fail_mask
 * with a bit outside TGSIM_FLOW_FB_REFUSALS is -EINVAL with a tgsim_last_error text that names
 * fail_mask and its value in hex.  fail_mask == 0 is legal: the flows are counted and never failed by
 * a verdict. */
int tgsim_flow_init_fb(void* engine, const tgsim_flow* p, const tgsim_flow_cc* cc, const tgsim_flow_rto* rto,
                       const tgsim_flow_fb* fb, const tgsim_flow_spec* flows, uint64_t n_flows);
/* The fb rows of flows [first, first + n), and the fb summary reduced on the device.  -EINVAL
 * ("verdict feedback is not armed") when flows are armed without fb or not at all; otherwise they
 * synchronize, and fail, like tgsim_flow_rto_rows and tgsim_flow_rto_report. */
int64_t tgsim_flow_fb_rows(void* engine, uint64_t first, uint64_t n, tgsim_flow_fb_row* out, size_t cap);
int     tgsim_flow_fb_report(void* engine, tgsim_flow_fb_summary* out);

/* ---- flow driver over shards ---------------------------------------------------------------- */
/* tgsim_flow_init_fb on an engine that owns peers [shard_begin, shard_end), which may be every peer.
 * `flows` is the WHOLE run's table, the same on every shard: it is replicated like the peer tables and
 * the ping targets, because a receiver's shard validates a data record against the sender's flow
 * (dst == r, seg < n_seg), which it does not own (16 B per flow, and first[] / cnt[] at 8 B per peer,
 * per shard).  Every field rule, -EINVAL text and -EBUSY rule of tgsim_flow_init_fb holds, less the
 * ownership test; cc, rto and fb are each NULL or not.  The table is sorted by src, so the flows an
 * engine owns (those whose src it owns) are one contiguous range [first, first + n) of it, possibly
 * empty (tgsim_flow_owned); the per-flow state -- the row, the bitmap, the due / attempt / sent rings,
 * the cc, rto and fb rows -- exists for them only.  (engine, NULL, NULL, NULL, NULL, NULL, 0) disarms,
 * frees the state and drops a generated window of its own that is still pending (the window of a step
 * the ranks refused, see the late rule); tgsim_flow_init(engine, NULL, NULL, 0) disarms either form.
 *
 * Every rule of the sections above holds.  What differs is where things happen:
 *   Offers   of flow f, its timers and its failing by tick: the shard that owns f.src (tgsim_gen_flow
 *            generates the owned sources' rows and involves no collective).
 *   Verdicts the feedback fold of flow f: f.src's shard, from the generated window's own rows and
 *            verdict bytes.
 *   ACK      a calendar entry is made from a delivered data record addressed to r at the shard that
 *            owns r, where the exchange's delivery emits the record; it becomes r's ACK there.
 *   Receipt  a delivered ACK addressed to q changes sender state at q's shard.
 *   Counters dup_ignored and corrupt_ignored count at the shard that emits the record; pending_acks
 *            is that shard's calendar.
 *   Order    unchanged: a window's verdicts take effect before the records the same step emits are folded.
 * While armed through this call the closed steps are accepted exactly as for the sharded ping driver:
 * tgsim_comm_step, tgsim_comm_launch / tgsim_comm_finish and, underneath them, tgsim_step_sim,
 * tgsim_step_sim_launch / _finish / _counts, tgsim_deliver / tgsim_deliver_async and
 * tgsim_deliver_slotted_async with one window; tgsim_step on an engine that owns every peer gives the
 * results of the unsharded form.  tgsim_comm_run, tgsim_step_sim_launch_slotted called directly and
 * tgsim_step_sim_launch_slotted_n stay -EBUSY (pipelined or fused: they cannot be closed-loop); one
 * generated window at a time, and none between tgsim_comm_launch and its tgsim_comm_finish (-EBUSY:
 * the window's receipts come first).
 *
 * The calendar of a shard holds the ACKs of data other shards offered, which it never sees offered: it
 * is grown, where needed, ahead of each delivery's receipts to what the last generation kept plus every
 * record received since (an entry is made from exactly one received record).  -ENOSPC stays the net.
 *
 * tgsim_flow_report, tgsim_flow_cc_report, tgsim_flow_rto_report and tgsim_flow_fb_report give THIS
 * shard's flows.  Reports merge over the shards field by field: every field by sum and hist by sum, bin
 * by bin, except fct_min_ns, cwnd_min, srtt_min and rto_min by min, and fct_max_ns, cwnd_max, srtt_max
 * and rto_max by max (a shard with nothing to report gives the neutral values it gives today:
 * UINT64_MAX for a minimum, 0 for a maximum).  tgsim_comm_flow_report does that on the device.
 * tgsim_flow_rows and its _cc / _rto / _fb forms take global flow indices inside the owned range
 * (-EINVAL, naming both ranges, otherwise).
 *
 * The late rule and the calendar overflow across ranks are the sharded ping driver's, word for word: one
 * rank's tgsim_gen_flow sees a late ACK or a late released segment (-EINVAL; nothing generated, no state
 * changed, the error stays); every rank still calls tgsim_comm_step / tgsim_comm_launch for every window;
 * with more than one rank the launch first agrees on the ranks' fault words (one 8-byte max all-reduce
 * and one host wait per window); when any rank is late EVERY rank's call returns -EINVAL,
 * tgsim_last_error names the rank and the tick, nothing is simulated, and the error stays on every rank
 * until it re-arms.  The reports stay readable.  A full calendar (-ENOSPC) is agreed the same way. */
int tgsim_flow_init_sharded(void* engine, const tgsim_flow* p, const tgsim_flow_cc* cc, const tgsim_flow_rto* rto,
                            const tgsim_flow_fb* fb, const tgsim_flow_spec* flows, uint64_t n_flows);
/* The owned flows: the contiguous range of the table whose src this engine owns (the whole table on an
 * engine that owns every peer, armed through either form).  -EINVAL when the driver is not armed. */
int tgsim_flow_owned(void* engine, uint64_t* first, uint64_t* n);
/* The WHOLE run's reports on every rank (collective, after tgsim_comm_init): each rank's local
 * reports are packed on the device into three runs (sums and histogram bins, minima, maxima), reduced
 * by three u64 all-reduces (sum, min, max) on the exchange stream and unpacked; no per-flow table
 * crosses between GPUs or to the host.  cc / rto / fb: NULL, or a buffer for a part that is armed (a
 * buffer for an unarmed part is -EINVAL naming the part, before any collective).  Returns n_bins;
 * -EINVAL without a communicator or when the driver is not armed through tgsim_flow_init_sharded,
 * -EBUSY between tgsim_comm_launch and tgsim_comm_finish, -ETIMEDOUT as the other collectives.  With
 * one rank it equals the local reports. */
int64_t tgsim_comm_flow_report(void* engine, tgsim_flow_summary* out, uint64_t* hist, size_t hist_cap,
                               tgsim_flow_cc_summary* cc, tgsim_flow_rto_summary* rto, tgsim_flow_fb_summary* fb);

/* ---- per-group traffic matrix (who offered what to whom, and what became of it) -------------- */
/* Every peer belongs to one group (a region, a composition group); the engine folds each window's
 * traffic into a matrix of (group of src, group of dst) cells on the device, whoever made the traffic
 * (tgsim_submit, tgsim_gen_storm, the gossip and ping drivers, bridge datagrams), so no delivery and
 * no per-instance table has to reach the host.  Words of a cell:
 *    0      offered packets (originals), since arming or the last reset
 *    1      offered bytes (len)
 *    2..9   verdict counts 0..7: the low nibble of every verdict byte, plus the high nibble when it
 *           is not TGSIM_V_NONE (the rule of TGSIM_METRICS_SRC columns 2..9)
 *    10     delivered records
 *    11     delivered bytes
 *    12     delivered records with TGSIM_FLAG_DUP
 *    13     delivered records with TGSIM_FLAG_CORRUPT
 * Words 0..9 are counted at the source's shard when the window is simulated, words 10..13 at the
 * destination's shard when a step emits the record (when tgsim_drain would show it).  A record purged
 * as lost_in_flight, or flushed, is never delivered: word 2 can stay above word 10.  The column
 * gd == n_groups is TGSIM_EXTERNAL (its words 10..13 are always 0).  The matrices of the shards of
 * one run merge by plain sum.
 * While armed, tgsim_step_n runs its windows one by one and tgsim_step_sim_launch_slotted_n returns
 * -EINVAL (as with TGSIM_OPT_METRICS: nothing is folded inside a fused launch); unlike
 * TGSIM_OPT_METRICS the report leaves the sparse windows' direct destination buckets on. */
#define TGSIM_GROUP_MAX   64u   /* groups per run */
#define TGSIM_GROUP_WORDS 14u
/* Arms the report: group_of[n_peers] (every entry < n_groups, 1 <= n_groups <= TGSIM_GROUP_MAX), the same
 * table on every shard.  Zeroes the matrix.  (engine, NULL, 0) disarms and frees.  Re-arming replaces
 * the table and zeroes.  -EINVAL (with a tgsim_last_error text) for n_groups 0 or above
 * TGSIM_GROUP_MAX, a NULL table with n_groups != 0, or an entry >= n_groups (the text names the
 * peer); -EBUSY while launched steps, generated windows or host packets are pending. */
int tgsim_groups_init(void* engine, const uint16_t* group_of, uint32_t n_groups);
/* out[(gs * (n_groups + 1) + gd) * TGSIM_GROUP_WORDS + w]; column gd == n_groups is TGSIM_EXTERNAL.
 * reset != 0 zeroes the matrix behind the copy, in stream order (interval series).  Returns the words
 * written (n_groups * (n_groups + 1) * TGSIM_GROUP_WORDS); -ENOSPC when cap is smaller; -EINVAL ("not
 * armed") on an engine without the report.  Synchronizes like tgsim_stats. */
int64_t tgsim_group_matrix(void* engine, uint64_t* out, size_t cap, int reset);

/* ---- packet capture of watched instances (tcpdump on a handful of peers) --------------------- */
/* For up to TGSIM_CAPTURE_MAX_PEERS watched peers the engine keeps two record lists on the device,
 * whoever made the traffic (tgsim_submit, tgsim_gen_storm, the gossip, ping and flow drivers, bridge
 * datagrams) and whether or not deliveries are kept (TGSIM_OPT_DISCARD_DELIVERIES): every packet a
 * watched peer offered with its verdict byte (TX), and every record delivered to it (RX).
 * DESIGN.md §5.12.  The order is fixed by construction:
 *   TX  after each window's simulation, for each watched peer this engine owns as a source, in
 *       ascending peer order, one record per offered packet of its row, in the row's order.  A netem
 *       clone makes no TX record of its own: it is the high nibble of the verdict byte.
 *   RX  after each window's delivery, for each watched peer this engine owns as a destination, in
 *       ascending peer order, the records delivered to it in drain order (t_ns, src, seq, clone
 *       first).  A record flushed or lost in flight is never delivered and has no RX record.
 * Windows append in window order.  With deliveries kept, a window's RX capture is that window's drain
 * filtered to the watched destinations, record for record, and its TX capture the window's packets
 * and verdict bytes filtered to the watched sources.  Shards own ascending contiguous ranges, so the
 * per-window reads of a run's ranks concatenated in rank order are the single engine's.
 * Room: each direction is one linear buffer of `cap` records.  A window's records are placed in
 * capture order while room remains, so what is kept is always a prefix of the capture stream; the
 * rest only counts in `dropped`.  Nothing is overwritten and no error is raised; a read empties the
 * direction.  seen == records read so far + pending + dropped, per direction, at every read.
 * While armed, tgsim_step_n runs its windows one by one and tgsim_step_sim_launch_slotted_n returns
 * -EINVAL (as with TGSIM_OPT_METRICS and the group matrix: nothing is captured inside a fused
 * launch); the sparse windows' direct destination buckets stay on.  An engine that never arms the
 * capture launches nothing for it. */
#define TGSIM_CAPTURE_MAX_PEERS 1024u
enum tgsim_capture_dir { TGSIM_CAPTURE_TX = 0, TGSIM_CAPTURE_RX = 1 };
typedef struct {            /* 32 B */
    uint64_t t_ns;          /* TX: (window start tick + the packet's tick) * tick_ns; RX: the record's delivery time */
    uint32_t src, dst, seq;
    uint16_t len;
    uint16_t flags;         /* RX: TGSIM_FLAG_*; TX: 0 */
    uint8_t  verdict;       /* TX: the packet's verdict byte (both nibbles); RX: 0 */
    uint8_t  dir;           /* enum tgsim_capture_dir */
    uint16_t _pad; uint32_t _pad2;
} tgsim_capture_rec;
typedef struct {            /* 56 B */
    uint64_t pending[2];    /* kept and not yet read, TX / RX */
    uint64_t seen[2];       /* records of watched, owned peers since arming, kept or not */
    uint64_t dropped[2];    /* of them, not kept for want of room */
    uint32_t n_watched, n_owned;
} tgsim_capture_info_t;
/* Arms the capture: peers[n], strictly ascending, 1 <= n <= TGSIM_CAPTURE_MAX_PEERS, every entry below
 * n_peers, the same list on every shard (an entry this engine does not own is accepted and ignored
 * there); tx_cap / rx_cap records of room, at most 2^31 each, 0 turns that direction off.  Re-arming
 * replaces the list, empties both buffers and zeroes the counters.  (engine, NULL, 0, 0, 0) disarms and
 * frees (a no-op on an unarmed engine).  -EINVAL, with a tgsim_last_error text that names the entry,
 * for an unsorted or repeated entry, an entry out of range, n of 0 or above the maximum, or both caps
 * 0; -EBUSY while launched steps, generated windows or host packets are pending. */
int tgsim_capture_init(void* engine, const uint32_t* peers, uint32_t n, uint64_t tx_cap, uint64_t rx_cap);
/* The counters, after every window issued so far.  -EINVAL ("capture is not armed") when unarmed. */
int tgsim_capture_info(void* engine, tgsim_capture_info_t* out);
/* Copies everything pending of direction dir, empties that direction and returns the count.  With
 * out == NULL and cap == 0: the pending count, nothing removed.  -ENOSPC when cap is below the pending
 * count (nothing removed); -EINVAL when unarmed or for dir > 1.  Synchronizes like tgsim_group_matrix
 * and returns a sticky simulation error as it does. */
int64_t tgsim_capture_read(void* engine, uint32_t dir, tgsim_capture_rec* out, size_t cap);

/* ---- sync counters (sync-service SignalEntry / Barrier) ------------------------------------ */
/* K7: TGSIM_SYNC_STATES u64 counters in device memory, incremented by a kernel on the engine's sync
 * stream (never behind a queued simulation) that also writes the new value into a pinned host
 * mirror, so polling a barrier reads host memory and never calls the device. */
#define TGSIM_SYNC_STATES 65536u
/* Increments state `state` by n and returns the new value (1-based sequence, SignalEntry). */
int64_t tgsim_signal(void* engine, uint32_t state, uint32_t n);
/* tgsim_signal without waiting for (or returning) the new value: bulk signals such as n instances
 * entering a barrier at once.  0 on success. */
int tgsim_signal_async(void* engine, uint32_t state, uint32_t n);
/* Returns 1 when the state's count >= target, 0 otherwise (after every signal issued so far). */
int tgsim_barrier_poll(void* engine, uint32_t state, uint64_t target);
/* The device counter table (TGSIM_SYNC_STATES u64, device memory) for a collective over the
 * shards (the sum over ranks is the global count); `event` (a hipEvent_t, may be null) is recorded
 * on the sync stream after every signal issued so far, for the collective's stream to wait on. */
int tgsim_sync_counters(void* engine, void** d_table, uint32_t* n_states, void* event);

/* ---- metrics (the plans' runenv counters/histograms, pkg/metrics viewer.go:46) ---- */
/* With TGSIM_OPT_METRICS, every step folds per-instance counters and log2 histograms on the
 * device (accumulated since create).  tgsim_metrics copies one table and returns its word count:
 *   TGSIM_METRICS_SRC  [instance of this shard][12]: offered packets, offered bytes, verdict
 *                      counts 0..7 (originals + clones), HTB records served, bytes served;
 *   TGSIM_METRICS_DST  [instance of this shard][2]: records and bytes delivered to it;
 *   TGSIM_METRICS_HIST [2][64]: per step, instances by netem backlog at the step end (ring +
 *                      queue), and by records delivered to them; bin b = floor(log2 x) + 1
 *                      (bin 0: none).
 * -ENODATA when the engine was created without TGSIM_OPT_METRICS. */
enum tgsim_metrics_kind { TGSIM_METRICS_SRC = 0, TGSIM_METRICS_DST = 1, TGSIM_METRICS_HIST = 2 };
#define TGSIM_METRICS_SRC_WORDS 12u
#define TGSIM_METRICS_DST_WORDS 2u
#define TGSIM_METRICS_BINS 64u
int64_t tgsim_metrics(void* engine, uint32_t kind, uint64_t* out, size_t cap);

/* ---- packet bridge: plan payloads through the simulated network ------- */
/* The payload bytes stay on the host; each datagram becomes a 16-B tgsim_pkt for the engine, and
 * every delivery the engine drains is handed back with its payload: twice for a netem duplicate,
 * with one bit flipped for a corrupted copy (the bit from a hash of (src, seq, clone)), never for
 * a lost, filtered or queue-full one.  Packet lengths seen by netem/HTB are payload + 28 B
 * (IPv4 + UDP headers).  Replaces the veth -> bridge hop of pkg/runner/local_docker.go:706-721 for
 * plans whose sockets are bridged (tgsim_udp_front below). */
typedef struct {
    uint64_t t_ns;  /* delivery time                                    */
    uint32_t src, dst, seq;
    uint16_t flags; /* TGSIM_FLAG_*                                     */
    uint16_t _pad;
    uint64_t off;   /* payload: data[off, off + len) of the recv buffer */
    uint32_t len;
    uint32_t _pad2;
} tgsim_msg;
/* The engine calls a bridge makes (NULL ops: this library's tgsim_* functions).  The CPU tests
 * drive the same bridge over the oracle's tgo_* functions. */
typedef struct {
    int (*submit)(void*, const tgsim_pkt*, size_t);
    int (*step)(void*, uint32_t);
    int64_t (*verdicts)(void*, uint8_t*, size_t);
    int64_t (*drain)(void*, tgsim_delivery*, size_t);
} tgsim_engine_ops;
int tgsim_bridge_create(void* engine, const tgsim_engine_ops* ops, uint32_t n_peers, uint32_t window_ticks,
                        uint64_t now_tick, void** out_bridge);
void tgsim_bridge_destroy(void* bridge);
/* Queues n datagrams: src[i] -> dst[i] (TGSIM_EXTERNAL allowed) with payload data[off[i], off[i+1]),
 * offered at absolute tick ticks[i] (ticks NULL: the start of the next window).  seq_out (may be
 * NULL) receives each datagram's per-source sequence number.  Returns n or -errno. */
int64_t tgsim_bridge_send(void* bridge, size_t n, const uint32_t* src, const uint32_t* dst, const uint8_t* data,
                          const uint64_t* off, const uint64_t* ticks, uint32_t* seq_out);
/* One window: submits the datagrams due in it, steps the engine, resolves every verdict and queues
 * every delivery with its payload.  Returns the deliveries queued. */
int64_t tgsim_bridge_step(void* bridge);
/* Moves up to max queued deliveries of `peer` (UINT32_MAX: of every peer, by destination) and their
 * payloads (packed into data, cap bytes) to the caller, oldest first; returns the count. */
int64_t tgsim_bridge_recv(void* bridge, uint32_t peer, tgsim_msg* msgs, size_t max, uint8_t* data, size_t cap);
int64_t tgsim_bridge_pending(void* bridge, uint32_t peer); /* deliveries queued (UINT32_MAX: all) */
int64_t tgsim_bridge_in_flight(void* bridge);              /* datagrams sent, not yet resolved  */
/* peer's data link was removed by the last tgsim_configure (tgsim_link_generation changed): every
 * datagram already handed to the engine that was sent by peer or addressed to it is resolved as
 * lost, since the engine flushes or purges it without a delivery.  Datagrams not yet handed to the
 * engine (due in a later window) are kept.  Returns how many were resolved. */
int64_t tgsim_bridge_link_removed(void* bridge, uint32_t peer);
uint64_t tgsim_bridge_now_tick(void* bridge);              /* start of the next window          */
/* UDP front end: one socket on 127.0.0.1 receives every instance's datagrams (a 4-byte big-endian
 * destination header, then the payload) from the instance's registered address; pump() moves what
 * arrived into the bridge (recvmmsg), steps one window and sends each delivery to its destination's
 * address with a 4-byte big-endian source header (sendmmsg). */
int tgsim_udp_front_create(void* bridge, uint16_t port, void** out_front);
int tgsim_udp_front_port(void* front);
int tgsim_udp_front_register(void* front, uint32_t peer, uint32_t ipv4, uint16_t port);
/* Header-less mode for unmodified UDP code: the front end binds a socket at (ipv4, port) (port 0:
 * any) that stands for peer's data address.  A registered instance that sends a plain datagram to
 * it sends to `peer` (no destination header); every delivery from `peer` leaves from that socket,
 * so the receiver's recvfrom sees peer's data address as the source (no source header).  Any
 * 127.0.0.0/8 address works without privileges.  Returns the bound port or -errno.  (TUN/TAP
 * capture, which would carry TCP too, needs /dev/net/tun and CAP_NET_ADMIN: DESIGN.md §9.) */
int tgsim_udp_front_bind_peer(void* front, uint32_t peer, uint32_t ipv4, uint16_t port);
int64_t tgsim_udp_front_pump(void* front);
void tgsim_udp_front_destroy(void* front);

/* ---- device timing (bench instrumentation) ------------------------------------------------ */
/* Average device time (ms) of the simulate kernel over the steps since the last reset, measured
 * with HIP events on the engine's stream. */
double tgsim_sim_kernel_ms(void* engine, uint64_t* n_launches, int reset);
/* The same for the delivery (K5: per-destination histogram scan, scatter, per-destination sort),
 * from its first kernel to its sort on the delivery stream, per window delivered (a fused group's
 * delivery counts each of its windows).  The span includes the time its kernels wait for CU slots
 * beside the next window's simulate kernel. */
double tgsim_delivery_kernel_ms(void* engine, uint64_t* n_windows, int reset);
void* tgsim_stream(void* engine);
/* Diagnostics: with TGSIM_STAMPS set at create time, the simulate kernel records 24 words per
 * workgroup (s_memrealtime at its phase boundaries, batch count, HW_ID, queue sizes); copies them
 * for the last step and returns the word count (0 when disabled). */
int64_t tgsim_debug_stamps(void* engine, uint64_t* out, size_t cap);
/* Diagnostics: HBM bytes the simulate kernels actually moved carrying netem queues and departure
 * rings between windows since the engine was created (loads + stores).  tgsim_stats_t's
 * queue_state_bytes models one load and one store per window; a fused group (tgsim_step_n) keeps
 * each source's queue in LDS across its windows and moves it once per group. */
int64_t tgsim_debug_carry_bytes(void* engine);
/* Diagnostics: records the simulate kernels wrote straight into destination buckets (sparse windows
 * of an engine that owns every peer) since the engine was created.  The others went
 * through the emit regions and the scatter. */
int64_t tgsim_debug_bucket_records(void* engine);
/* Diagnostics: windows simulated by fused launches (tgsim_step_n) since the engine was created. */
int64_t tgsim_debug_fused_windows(void* engine);
/* Diagnostics: fused launches (groups of windows) since the engine was created. */
int64_t tgsim_debug_fused_launches(void* engine);
/* Diagnostics: windows simulated by the sparse kernels (k_sim_sparse + k_sim_multi + k_sim_list) since
 * the engine was created; the others ran the dense k_sim (or were fused). */
int64_t tgsim_debug_sparse_windows(void* engine);
/* Diagnostics of a TGSIM_CHECK build of the engine (scripts/r05_check_build.sh): cross-lane reads whose
 * source lanes were inactive so far, process-wide.  -ENOSYS in the product build. */
int64_t tgsim_debug_exec_faults(void);

#ifdef __cplusplus
}
#endif

#endif /* TGSIM_H */
