/*
 * flipchain.h -- C-ABI of the MI355X-native flip-walk engine (libflipchain.so).
 *
 * This is the drop-in boundary for the reference's hot path: the gerrychain MarkovChain
 * protocol as the reference drives it,
 *
 *   exp_chain = MarkovChain(slow_reversible_propose_bi,
 *                           Validator([single_flip_contiguous, popbound]),
 *                           accept=cut_accept, initial_state=grid_partition,
 *                           total_steps=100000)          grid_chain_sec11.py:340-342
 *   for part in exp_chain: ...                           grid_chain_sec11.py:366-402
 *
 * Each entry point below names the reference interface it replaces.  Plain pointers and
 * sizes only; no C++ exceptions cross this boundary; every call returns an int status
 * (FC_OK = 0, < 0 error) and leaves a thread-local message in fc_last_error().
 *
 * Threading: one fc_run per host thread at a time.  The library has no global mutable
 * state besides the thread-local error string.  fc_run_steps is asynchronous on the given
 * HIP stream (NULL = the run's own stream); every fc_run_read_* call synchronises.
 *
 * Ownership: fc_graph_create / fc_run_create copy all host arrays; the library owns its
 * device buffers and frees them in *_destroy.
 */
#ifndef FLIPCHAIN_H
#define FLIPCHAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_OK 0
#define FC_ERR_ARG (-1)          /* bad argument (TypeError / IndexError analogues)        */
#define FC_ERR_INVALID_STATE (-2) /* initial state not valid: MarkovChain raises ValueError */
#define FC_ERR_HIP (-3)          /* HIP runtime failure or no GPU                           */
#define FC_ERR_UNSUPPORTED (-4)  /* configuration outside what the kernels implement        */
#define FC_ERR_NOMEM (-5)

/* fc_params.struct_size / abi_version: a caller built against another layout of fc_params is
 * rejected (FC_ERR_ARG) instead of read past.  Bumped whenever fc_params changes.           */
#define FC_ABI_VERSION 5u

/* fc_graph_create flags */
#define FC_GRAPH_NO_EXACT 0x1u   /* never trust the planar local contiguity rule            */

/* fc_params.proposal */
#define FC_PROPOSE_BI_SIGN 0     /* slow_reversible_propose_bi, grid_chain_sec11.py:132-145 */
#define FC_PROPOSE_PAIR 1        /* slow_reversible_propose,    grid_chain_sec11.py:117-130 */
#define FC_PROPOSE_RECOM 2       /* recom tree proposal built at grid_chain_sec11.py:328-335:
                                    spanning-tree bipartition of two merged districts       */

/* fc_params.diag_mask: per-yield driver diagnostics kept on the device
 * (grid_chain_sec11.py:350-419).  The streaming sums are always kept.                    */
#define FC_DIAG_WAIT 0x1u        /* geometric waits, geom_wait :147-148 -> wait.txt          */
#define FC_DIAG_HIST 0x2u        /* per-chain histograms of |cut| and |B| over yields        */
#define FC_DIAG_EDGES 0x4u       /* per-edge cut_times, :383-384                             */
#define FC_DIAG_FLIPS 0x8u       /* per-node num_flips / part_sum / last_flipped, :396-400   */
#define FC_DIAG_SERIES 0x10u     /* per-chain log of accepted flips (fc_event): the rce / rbn
                                    series of :367-369 in run-length form; feeds
                                    fc_run_autocorr and the slope / angle series (:371-392)  */
#define FC_DIAG_FLIPS_EXACT 0x20u /* the corrected companions of FC_DIAG_FLIPS (SURVEY App. A.6
                                    quirks 1-2): accepted flips per node, the time integral of
                                    each node's label over all yields, and the yield of its last
                                    accepted flip -- fc_run_read_flips_exact                   */

/* fc_params.accept: the accept callable (k = 2).  The variants are the reference's
 * alternatives, built but unused by its sweeps.                           */
#define FC_ACCEPT_CUT 0          /* cut_accept: random() < base ** (cut - cut'), :171-179     */
#define FC_ACCEPT_UNIFORM 1      /* uniform_accept: 1 if its constraints hold, :159-165        */
#define FC_ACCEPT_ANNEAL 2       /* annealing_cut_accept_backwards: random() <
                                    base ** (beta (cut - cut')) * |B'| / |B|, :81-110          */

/* Constraint sets (fc_params.con_valid / con_accept).  A constraint in con_valid is a
 * Validator member: a proposal failing it is re-drawn (no step).  One in con_accept is
 * tested inside the accept callable: failing it rejects the step (the state re-yields).  */
#define FC_CON_CONTIG 0x1u       /* single_flip_contiguous                                  */
#define FC_CON_POP 0x2u          /* within_percent_of_ideal_population (pop_lo / pop_hi)   */
#define FC_CON_BOUNDARY 0x4u     /* boundary_condition, :43-52: both districts keep a node of
                                    the outer face (the reference's boundary_node set)      */
#define FC_CON_FIXED 0x8u        /* fixed_endpoints, :39-40: pinned edges stay cut; passed as
                                    the pinned edges' endpoints (`frozen`), which may not flip */
#define FC_CON_EMPTY 0x100u      /* con_valid: an empty Validator (0 selects CONTIG | POP)   */

/* fc_params.flags */
#define FC_FLAG_FORCE_BFS 0x1u   /* resolve every multi-run contiguity case by device BFS   */
#define FC_FLAG_SERIES_TWO_PASS 0x2u /* fc_run_frame_series_changes: the two-pass form (count, then
                                    write at the offsets) instead of one staged pass -- the form a
                                    run whose staging exceeds a tenth of free device memory takes;
                                    same output (a cross-check)                                 */
#define FC_FLAG_TALLY_LOG_SMALL 0x4u /* k = 2 full diagnostics: a 64-entry tally log per chain, so
                                    chains fill it and apply the rest of a launch's tallies with
                                    atomics -- the path a device short of memory takes; same
                                    output (a cross-check)                                      */
#define FC_FLAG_NB_PAIRS 0x8u    /* k > 2 PAIR runs: |b_nodes| (stats nb / sum_nb, the |B| histogram,
                                    geom_wait's p = |b_nodes| / (N^k - 1)) counts the (node,
                                    district) pairs of the pair updater b_nodes (:151-153), which a
                                    k > 2 driver running slow_reversible_propose (:117-130)
                                    registers as "b_nodes", instead of the nodes of b_nodes_bi
                                    (:155-156).  The histogram and log1mp then have
                                    fc_run_nb_width entries; no-op for k = 2.  Such runs commit
                                    one flip at a time (tune_multi_flip has no effect)           */
#define FC_FLAG_VOTES_GLOBAL_CUR 0x10u /* fc_run_election_series: the replay keeps each chain's
                                    current assignment in a global row instead of LDS -- the path a
                                    graph too large for the default dynamic LDS limit takes; same
                                    output (a cross-check)                                      */

typedef struct fc_graph fc_graph;
typedef struct fc_run fc_run;

typedef struct fc_graph_info {
    int32_t n_nodes;
    int32_t n_edges;
    int32_t ring_max;     /* entries per node record (8 or 16)                            */
    int32_t max_degree;
    int32_t n_exact;      /* nodes whose local contiguity rule is exact (k = 2)          */
    int32_t n_gamma;      /* nodes on the outer face                                      */
    int32_t planar;       /* positions given and no two edges cross                       */
    int32_t outer_simple; /* outer face boundary is a simple cycle                        */
} fc_graph_info;

typedef struct fc_params {
    uint32_t struct_size;      /* sizeof(fc_params) as the caller compiled it (fc_params_init) */
    uint32_t abi_version;      /* FC_ABI_VERSION as the caller compiled it                  */
    int32_t k;                 /* districts: 2 (BI_SIGN or PAIR) or 3..32 (PAIR)            */
    int32_t proposal;          /* FC_PROPOSE_*                                              */
    double base;               /* cut_accept base when `bases` is NULL (:171-179, :279-280) */
    int64_t pop_lo, pop_hi;    /* inclusive integer bounds equivalent to
                                  within_percent_of_ideal_population (:319); every chain's
                                  unless chain_pop_bounds is given                          */
    uint64_t seed;             /* Philox key (DESIGN.md "Random stream")                    */
    uint32_t chain_id_offset;  /* global id of local chain 0 (multi-GPU sharding)           */
    uint32_t diag_mask;        /* FC_DIAG_*                                                 */
    uint32_t flags;            /* FC_FLAG_*                                                 */
    int32_t device;            /* HIP device ordinal                                        */
    int32_t trace_chains;      /* chains 0..trace_chains-1 record per-proposal traces      */
    int64_t trace_cap;         /* records per traced chain                                  */
    const int32_t *labels;     /* [k] reference district labels (e.g. -1, 1); NULL = 0..k-1 */
    const double *log1mp;      /* [n+1] log(1 - b/(N^k - 1)) ([fc_run_nb_width] with
                                  FC_FLAG_NB_PAIRS); NULL = computed in double               */
    int32_t wmax;              /* PAIR: district slots per node draw (<= 0: min(max deg, k-1)) */
    int32_t hit_lo, hit_hi;    /* hitting time: first yield with hit_lo <= |cut| <= hit_hi
                                  (hit_lo > hit_hi: off)                                     */
    int64_t event_cap;         /* FC_DIAG_SERIES: events kept per chain per series window: one
                                  per accepted flip; a ReCom run logs one per node an accepted
                                  step moves (its move log), so (steps in the window) * n always
                                  suffices (the measured mean: DESIGN.md "ReCom move log")   */
    /* accept / constraint variants (k = 2; all zero = Validator([single_flip_contiguous,
       popbound]) + cut_accept, the reference's configuration)                               */
    int32_t accept;            /* FC_ACCEPT_*                                                */
    uint32_t con_valid;        /* FC_CON_* in the Validator (0 = CONTIG | POP)               */
    uint32_t con_accept;       /* FC_CON_* tested by the accept callable                      */
    double beta;               /* FC_ACCEPT_ANNEAL exponent factor (the reference: 5)       */
    const int32_t *frozen;     /* FC_CON_FIXED: [n_frozen] endpoints of the pinned edges    */
    int32_t n_frozen;
    /* FC_PROPOSE_RECOM: recom(pop_target, epsilon, node_repeats) [gc-0.2]; the Validator is
       the population bound, acceptance is cut_accept with `base` (1: always_accept).  The
       graph has at most 8000 nodes and a population total of at most INT32_MAX (2^31 - 1);
       fc_run_create answers FC_ERR_UNSUPPORTED otherwise                                    */
    double recom_pop_target;
    double recom_epsilon;
    int32_t recom_node_repeats;  /* roots tried per spanning tree (<= 0: 1)                */
    int32_t recom_max_attempts;  /* roots tried per proposal before giving up (<= 0: 10000) */
    /* Launch tuning.  Scheduling only: no trajectory, statistic or trace depends on these
     * (tests/test_parity_gpu.py::test_sec11_batch_shapes, test_pair_gpu.py::test_k4_wait_queue_lengths). 0 = the default;
     * the library reads no environment variables.                                          */
    int32_t tune_nsub;          /* draws per batch in units of 64, in {1, 2, 4}: k = 2 default 4
                                   (a window of 64 nsub draws, four node words per Philox call;
                                   band stream: rounds of 64); k > 2 default 2 (4 when the slot
                                   bound wmax exceeds 8); anything else FC_ERR_ARG              */
    int32_t tune_hit_stop;      /* rounds of 64 (k > 2, k = 2 band stream): no further round
                                   once a batch holds this many boundary hits (default 32).
                                   The k = 2 node stream has no rounds (a 64 * nsub window closed
                                   by the 64th hit): nonzero there is FC_ERR_ARG                */
    int32_t tune_par_min;       /* k = 2: segment-parallel commit from this many acceptances on
                                   (default 3; > 64 = one event at a time)                     */
    int32_t tune_wait_queue;    /* accepted states queued for their geometric wait before one
                                   full-width draw pass (default and maximum: 64 for k = 2, 32
                                   for k > 2)                                                  */
    int32_t tune_chains_per_block; /* chains (wavefronts) per workgroup: 1 (default), 2 or 4   */
    int32_t tune_prio_div[3];   /* k = 2 SIMD issue priority 1/2/3 for chains with |B| below
                                   n / div (default {2, 5, 10}); tune_prio_div[0] < 0: off      */
    float tune_prio_th[3];      /* ... and, once a chain has taken 1/16 of the launch's steps,
                                   for projected finish / previous launch's slowest above these
                                   (default {0.95, 1.0, 1.05}); tune_prio_th[0] < 0: |B| rule only */
    int32_t tune_search_waves;  /* k > 2, chains of more than 16 KB LDS whose contiguity needs the
                                   device search (no district-graph rule): 4 = one chain per
                                   256-thread workgroup, searches by the whole workgroup;
                                   1 = one-wave workgroups, wave search (default: faster on
                                   the short searches of C4 / C5)                */
    int32_t tune_deal;          /* k = 2 chain dealing: each SIMD runs one chain of every quarter
                                   of the previous launch's draws (most first) instead of the
                                   dispatcher's order; 1 = on, -1 = off (default).  Changes
                                   which wave runs which chain, never a trajectory              */
    /* Per-chain configuration.  The reference sweeps population tolerance x base x alignment
     * (grid_chain_sec11.py:182-184); with per-chain bases (fc_run_create `bases`) and bounds the
     * whole sweep is one run.                                                                   */
    const int64_t *chain_pop_bounds; /* [2 * n_chains]: chain c's inclusive (pop_lo, pop_hi), or
                                        NULL for pop_lo / pop_hi                                 */
    /* Node stream of k = 2 runs.  Both are rejection sampling of the reference's
     * random.choice(list(b_nodes)) (grid_chain_sec11.py:143), so the chain's law is the same;
     * the trajectories differ.  FC_STREAM_NODE (0): a draw picks one of all n nodes.
     * FC_STREAM_BAND: a draw picks the i-th node (ascending) of the band S = b_nodes plus their
     * neighbours, which the chain keeps lazily: after an accepted flip that puts a node outside
     * S into b_nodes, S is rebuilt from that state.  Short boundaries then waste few draws.
     * k = 2, n <= 4096, no replay tape; oracle: fr_params.stream                               */
    int32_t stream;
    int32_t tune_multi_flip;    /* k > 2 with the district-graph rule: commit several independent
                                   accepted flips per pass (0: auto = on; 1: on; -1: one at a
                                   time; 2: on with the hashed neighbour marks; 3: on with exact
                                   marks, one LDS byte per node -- on (0 / 1) takes the exact marks
                                   when they cost no residency, fc_run_kernel_name shows which).
                                   Scheduling only, like every tune_* field                    */
    int32_t tune_ring_table;    /* k = 2, rings of at most 8 cells, graphs without a node of more
                                   than four neighbours: the ring verdicts of a proposal are read
                                   from a table of (ring class, ring bits), built once per run,
                                   when the graph's rings fall into at most this many classes
                                   (distinct length / neighbour / link masks; 512 B per class).
                                   Unlike the other tune_* fields 0 is a value, not the default:
                                   0 = no table (the arithmetic), fc_params_init sets 64; at most
                                   255.  A caller that zero-fills the struct instead of calling
                                   fc_params_init gets no table, and with it the kernel's ring body
                                   (about a tenth slower on sec11): set 64.  Scheduling only:
                                   both forms give the same verdicts                             */
} fc_params;

#define FC_STREAM_NODE 0
#define FC_STREAM_BAND 1

/* Zero *p, then set struct_size / abi_version and the defaults a zeroed struct does not give:
 * k = 2, base 1, pop bounds [0, INT32_MAX], hitting-time window off.  FC_ERR_ARG when struct_size is
 * not this library's sizeof(fc_params) (the caller's header is another version).            */
int fc_params_init(fc_params *p, uint32_t struct_size);

/* Per-chain statistics.  "Yields" are the states a `for part in exp_chain` loop sees:
 * the initial state plus one per valid step; every sum runs over all yields. */
typedef struct fc_chain_stats {
    int64_t steps;        /* valid steps (MarkovChain steps after the initial yield)      */
    int64_t proposals;    /* proposals: draws that hit a boundary node                    */
    int64_t draws;        /* raw random draws                                             */
    int64_t accepted;
    int64_t inv_contig;   /* rejected by single_flip_contiguous                           */
    int64_t inv_pop;      /* rejected by the population bound                             */
    int64_t sum_cut;      /* sum over yields of |cut_edges|       (rce)                   */
    int64_t sum_nb;       /* sum over yields of |b_nodes|         (rbn)                   */
    int64_t sum_wait;     /* sum over yields of geom              (wait.txt)              */
    int64_t sum_cut2;
    int64_t sum_nb2;
    int64_t wait_cur;     /* geometric wait of the current state                          */
    int64_t bfs_calls;    /* contiguity cases resolved by device BFS                      */
    int64_t bfs_levels;
    int32_t cut;          /* current |cut_edges|                                           */
    int32_t nb;           /* current |b_nodes|                                             */
    int32_t last_flip;    /* node flipped to create the current state (-1: initial)       */
    int32_t stuck;        /* a launch hit max_draws before finishing its steps            */
    int64_t hit_time;     /* first yield index with |cut| in [hit_lo, hit_hi], -1: not yet  */
    int64_t events;       /* events in the current series window (may exceed cap): accepted flips;
                             for a ReCom run with a move log, the nodes its accepted steps moved */
    int64_t series_t0;    /* yield index at which the series window starts                */
    int32_t series_cut0;  /* |cut| of that yield                                           */
    int32_t series_nb0;   /* |B| of that yield                                             */
} fc_chain_stats;

/* One accepted flip (FC_DIAG_SERIES): yield t is the first state with a[v] = target;
 * |cut| and |B| hold from yield t until the next event's t (16 B).
 * A ReCom run with a move log writes one event per node an accepted step moves: a burst of events
 * in ascending v that share t, cut and nb (those of the step's new state).  An accepted step that
 * reproduces the plan, like a rejected one, writes nothing. */
typedef struct fc_event {
    int64_t t;
    uint16_t v;
    uint16_t cut;
    uint16_t nb;
    uint8_t target;
    uint8_t reserved;
} fc_event;

/* One record per proposal (trace mode), identical in layout to the oracle's. */
typedef struct fc_record {
    int64_t draw;
    int32_t v;
    int32_t flags;        /* 1 valid, 2 accepted, 4 invalid: contiguity, 8 invalid: pop   */
    int32_t cut;          /* state after this proposal                                     */
    int32_t nb;
    int64_t wait;         /* geometric wait of the yielded state (valid proposals)        */
} fc_record;

/* One ReCom proposal (trace mode, FC_PROPOSE_RECOM), identical in layout to the oracle's. */
typedef struct fc_recom_record {
    int64_t draw;
    int32_t edge;         /* cut edge chosen (canonical edge id): its two districts merge   */
    int32_t root;         /* spanning-tree root of the successful attempt                   */
    int32_t child;        /* the cut's child: subtree(child) -> district of edge's first end */
    int32_t attempts;     /* roots tried                                                     */
    int32_t flags;        /* 1 valid, 2 accepted, 8 invalid: population                      */
    int32_t cut;          /* |cut edges| after the proposal                                  */
} fc_recom_record;

/* ---- graph: replaces gerrychain Graph + the networkx lattice (:186-260) ------------ */
/* CSR adjacency (symmetric, no self loops), node populations (Tally('population'),
 * :299), optional planar positions [2n] from which the per-node link rings and the
 * exactness of the local contiguity rule are derived. */
int fc_graph_create(int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *pop,
                    const double *pos_xy, uint32_t flags, fc_graph **out);
int fc_graph_get_info(const fc_graph *g, fc_graph_info *out);
/* Canonical edge list (u < v, CSR order): the order of cut_times / cut_edges. */
int fc_graph_edges(const fc_graph *g, int32_t *eu, int32_t *ev);
/* Debug export of the rings: entries [n * ring_max] (padded with the node itself) and
 * meta [n] (bits 0-7 length, 8 exact, 9 outer-face, 16-31 neighbour mask, 32-47 link mask). */
int fc_graph_rings(const fc_graph *g, int32_t *ring, uint64_t *meta);
void fc_graph_destroy(fc_graph *g);

/* ---- seed plans: random k-district start plans, gerrychain's recursive_tree_part [gc-0.2] on
 * the device.  A function of the graph: no run is needed, the call is synchronous.
 * Plan G = plan_id_offset + local index, attempt r = 0 .. max_restarts: every node starts in
 * district k - 1 (the remainder M); level i = 0 .. k - 2 runs the ReCom proposal's bipartition_tree
 * on M (the same spanning tree, root and child choices, Philox draw index
 * 0xFFFFFFFF00000000 | r << 8 | i, chain word G, key seed -- an index no run's draw counter reaches)
 * with the integer cut rule: node x != root is a cut iff  pop_lo <= s <= pop_hi  and
 * m pop_lo <= pop(M) - s <= m pop_hi,  s = pop(subtree(x)), m = k - 1 - i the districts the
 * remainder must still hold.  subtree(child) becomes district i.  A level without a cut after
 * max_attempts attempts fails the attempt, and attempt r + 1 starts from scratch; a plan that fails
 * at r = max_restarts has ok = 0 and a row of -1.  Every ok plan has k connected districts inside
 * [pop_lo, pop_hi], and depends on (graph, k, pop_lo, pop_hi, seed, G, node_repeats, max_attempts,
 * max_restarts) only: not on how plans are split over calls or devices.                         */
typedef struct fc_seed_params {
    uint32_t struct_size;      /* sizeof(fc_seed_params) as the caller compiled it (fc_seed_params_init) */
    uint32_t abi_version;      /* FC_ABI_VERSION as the caller compiled it                  */
    int32_t k;                 /* districts, 2..32                                          */
    int64_t pop_lo, pop_hi;    /* inclusive integer bounds of every district (fc_params.pop_lo / pop_hi) */
    uint64_t seed;             /* Philox key                                                */
    uint32_t plan_id_offset;   /* global id of local plan 0                                 */
    int32_t device;            /* HIP device ordinal                                        */
    int32_t node_repeats;      /* roots tried per spanning tree; 0: 1                       */
    int32_t max_attempts;      /* attempts per level; 0: 256                                */
    int32_t max_restarts;      /* restarts per plan; 0: 16                                  */
} fc_seed_params;
typedef struct fc_seed_stats {
    int64_t attempts, trees;   /* totals over all levels and restarts                       */
    int32_t restarts;          /* the attempt r the plan ended in                           */
    int32_t ok;                /* 1: a valid plan; 0: failed (row of -1, cut = nb = 0)      */
    int32_t cut, nb;           /* |cut edges| and |boundary nodes| of an ok plan            */
} fc_seed_stats;
/* Zeroes *p and sets struct_size / abi_version and k = 2, pop_hi = INT64_MAX. */
int fc_seed_params_init(fc_seed_params *p, uint32_t struct_size);
/* n_plans plans into assign_out (rows packed to n bytes); stats_out and kernel_ms (the kernel's
 * device time, HIP events) may be NULL.  Checked on the host before any device call: FC_ERR_ARG for
 * k outside [2, 32], pop_lo > pop_hi, k pop_lo > the population total or k pop_hi < it, n_plans < 0,
 * negative node_repeats / max_attempts / max_restarts, max_restarts >= 2^24, or a struct_size / abi_version of
 * another header; FC_ERR_UNSUPPORTED for n > 8000, a population total above INT32_MAX, a node degree
 * above 16 or a disconnected graph.  FC_ERR_NOMEM when the plan rows and tables exceed a tenth of
 * the free device memory: split the call (plan_id_offset keeps the plans the same).            */
int fc_graph_seed_plans(const fc_graph *g, const fc_seed_params *p, int32_t n_plans,
                        int8_t *assign_out,       /* [n_plans * n], 0..k-1, -1 rows for failed plans */
                        fc_seed_stats *stats_out, /* [n_plans] or NULL */
                        float *kernel_ms);        /* or NULL */
/* The kernel instance the calling thread's last fc_graph_seed_plans call launched, spelled as
 * rocprofv3 reports it ("" before the first). */
int fc_seed_kernel_name(char *buf, int32_t cap);

/* ---- run: replaces Partition(graph, assignment, updaters) + MarkovChain(...) --------- */
/* init_assign: [n_chains * n] district ids 0..k-1 (one initial plan per chain).
 * bases: [n_chains] per-chain cut_accept base, or NULL for params->base.
 * Validates every initial state like MarkovChain.__init__ (FC_ERR_INVALID_STATE) against its
 * chain's population bounds.  FC_ERR_ARG when p->struct_size != sizeof(fc_params) or
 * p->abi_version != FC_ABI_VERSION (a caller compiled against another fc_params layout). */
int fc_run_create(const fc_graph *g, const fc_params *p, int32_t n_chains, const int8_t *init_assign,
                  const double *bases, fc_run **out);
/* Advance every chain by n_steps valid steps (the reference's step semantics: invalid
 * proposals are re-drawn and not counted).  max_draws caps the draws per chain per call
 * (<= 0: 64 * 1024 * n_steps); a capped chain sets stats.stuck.  Asynchronous. */
int fc_run_steps(fc_run *r, int64_t n_steps, int64_t max_draws, void *hip_stream);
/* Replay mode: chain c reads its random words from tape[c * n_draws * 6 ...] (6 u32 per
 * draw: 4 proposal words, 2 geometric words) instead of Philox.  NULL detaches. */
int fc_run_set_tape(fc_run *r, const uint32_t *tape, int64_t n_draws);
/* Replay of the initial state's geometric wait (geom_wait :147-148, drawn by numpy for the
 * yielded initial state in the reference): chain c's wait becomes the inversion of the 53-bit
 * uniform in words[2c], words[2c + 1] (same layout as tape words 4-5) instead of the
 * purpose-2 Philox draw.  Together with a node tape this replays a
 * trajectory of the reference's own random streams bit for bit.  Only before the first
 * fc_run_steps (FC_ERR_ARG after); needs FC_DIAG_WAIT.                                     */
int fc_run_set_initial_wait(fc_run *r, const uint32_t *words);
int fc_run_sync(fc_run *r);
/* Device time of the last fc_run_steps launch, from HIP events on its stream. */
int fc_run_last_ms(fc_run *r, float *ms);
/* Device times (ms) of every fc_run_steps launch since the previous call (up to cap;
 * *n receives the count); synchronises on the last launch and resets the record. */
int fc_run_timings(fc_run *r, float *ms, int32_t cap, int32_t *n);
int fc_run_read_stats(fc_run *r, fc_chain_stats *out);
int fc_run_read_state(fc_run *r, int8_t *assign_out);
/* District populations [c * k] (Tally('population'), :299). */
int fc_run_read_pops(fc_run *r, int64_t *pops_out);
int fc_run_read_trace(fc_run *r, int32_t chain, fc_record *out, int64_t cap, int64_t *len);
/* ReCom runs: the per-proposal records of a traced chain (*len may exceed cap). */
int fc_run_read_recom_trace(fc_run *r, int32_t chain, fc_recom_record *out, int64_t cap, int64_t *len);
/* Restart every traced chain's record buffer at 0 (chunked per-step iteration). */
int fc_run_trace_reset(fc_run *r);
int fc_run_read_hist(fc_run *r, int64_t *cut_hist, int64_t *nb_hist);      /* [c*(E+1)], [c*nb_width] */
int fc_run_read_edges(fc_run *r, int64_t *cut_times);                     /* [c*E], finalised     */
/* num_flips / part_sum / last_flipped [c*n], finalised as grid_chain_sec11.py:416-418. */
int fc_run_read_flips(fc_run *r, int64_t *num_flips, int64_t *part_sum, int64_t *last_flipped);
/* FC_DIAG_FLIPS_EXACT, [c*n] each (the statistics the driver's :396-400 / :416-418 aim at,
 * without its quirks; App. A.6):
 *   flip_count[u]  = accepted flips of u (the driver's num_flips counts every yield of the state
 *                    u's flip created, because part.flips is stale on rejected steps);
 *   occupancy[u]   = sum over all yields t of labels[a_t(u)] (the driver's part_sum drops the
 *                    final segment of every node that flipped at least once);
 *   last_accept[u] = yield index of u's last accepted flip (0: never flipped).
 * FC_ERR_ARG if FC_DIAG_FLIPS_EXACT is off; ReCom runs do not keep them (FC_ERR_UNSUPPORTED at
 * fc_run_create). */
int fc_run_read_flips_exact(fc_run *r, int64_t *flip_count, int64_t *occupancy, int64_t *last_accept);
/* Rao-Blackwellised companion of wait.txt (App. A.6 quirk 3: the cached geometric sample repeats
 * on rejected steps): out[c] = sum over yields of E[geom_wait | |B|] = (N^k - 1) / |B| - 1
 * (geom_wait :147-148), from the |B| histogram.  Needs FC_DIAG_HIST (FC_ERR_ARG otherwise). */
int fc_run_read_wait_expected(fc_run *r, double *out);
/* ---- series diagnostics (FC_DIAG_SERIES): the per-yield lists rce / rbn (:367-369) ----- */
/* The event log and every pass below serve flip runs and ReCom runs alike.  A ReCom run created
 * with FC_DIAG_SERIES and an event_cap keeps a move log (the kernel instance fc::recom_log_kernel);
 * one created without answers FC_ERR_UNSUPPORTED to the setters and series calls of the election,
 * compactness, locality-splits, plan-sample and heat-map sections (create it with FC_DIAG_SERIES and an
 * event_cap), and FC_ERR_ARG to fc_run_read_events and fc_run_autocorr, like any run without a log.
 * The burst convention: several events may share one t (the nodes one ReCom step moves), and
 *   a_t = the window-start assignment with every event of t_e <= t applied,
 * so the assignments between the events of one burst are not plans: they hold for no yield, weigh
 * nothing in any sum or histogram, and are never sampled.  |cut| and |B| at yield t are those of
 * the last event with t_e <= t.  A flip run's events have strictly increasing t. */
/* Events of one chain's current window (*len = events recorded, may exceed cap). */
int fc_run_read_events(fc_run *r, int32_t chain, fc_event *out, int64_t cap, int64_t *len);
/* Start a new window at the current yield (events dropped; hit_time is kept). */
int fc_run_series_reset(fc_run *r);
/* Autocorrelation of the |cut| series over the window's yields t0..steps, on the device:
 * lag_sums[c * nlags + j] = sum_t x_t x_{t + lags[j]} (exact int64), and, if acf != NULL,
 * acf[c * nlags + j] = sum_t (x_t - m)(x_{t+L} - m) / sum_t (x_t - m)^2 with m the window
 * mean (the biased sample ACF, statsmodels' acf default), formed on the host from exact
 * integer sums.  FC_ERR_ARG if a chain's event log overflowed event_cap. */
int fc_run_autocorr(fc_run *r, const int32_t *lags, int32_t nlags, int64_t *lag_sums, double *acf);
/* Frame-edge slope / angle series of chains [c0, c0 + nc) over the current window
 * (boundary_slope + the driver's loop body, grid_chain_sec11.py:55-78,371-394;
 * Frankenstein_chain.py:55-78,399-422).  k = 2 flip runs only (FC_ERR_UNSUPPORTED otherwise: the
 * outputs have an entry per event, which means nothing inside a ReCom burst).
 *   frame_u/v [n_frame <= 256]: the frame edges boundary_slope can return, in the order
 *                               whose first two cut members are used;
 *   mid_xy [2 n_frame]:          their midpoints (enda / endb) in the reference's node
 *                               coordinates; (cx, cy) the angle centre ((20, 20) there).
 * Output [i * cap + j] for chain c0 + i: j = 0 the window start yield, j >= 1 the state
 * created by event j - 1 (it holds for yields event.t .. next event.t - 1); entries j >= len[i]
 * are padding and left undefined (the outputs are copied whole from a device buffer):
 *   slope (+inf when the two midpoints share x), angle = arccos(clip(cos)), n_cut = frame
 *   cut edges (< 2: slope = angle = NaN, where the reference raises IndexError).
 * len[i] = events + 1.  FC_ERR_ARG when cap is too small or a log overflowed event_cap. */
int fc_run_frame_series(fc_run *r, int32_t c0, int32_t nc, int32_t n_frame, const int32_t *frame_u,
                        const int32_t *frame_v, const double *mid_xy, double cx, double cy, int64_t cap,
                        double *slope, double *angle, int32_t *n_cut, int64_t *len);
/* Change points of the same slope / angle series: what the reference's slope / angle plots
 * (grid_chain_sec11.py:476-484, plt.plot(slopes) / plt.plot(angles)) draw, without one entry
 * per event.  For chain c0 + i, entries offsets[i] .. offsets[i + 1] - 1 hold (t, slope,
 * angle): the values the per-yield lists (:382,394) take from yield t up to the next entry's t
 * (the last up to the current yield); the first entry is the window start, and every later one
 * is an event whose slope or angle differs (bitwise) from the previous entry's.  offsets
 * [nc + 1] is always filled; with t, slope and angle all NULL the call only sizes the output,
 * otherwise cap (entries per output array) must be >= offsets[nc] (FC_ERR_ARG, offsets still
 * filled, so a caller with buffers of a guessed size calls once and only re-calls on a miss).
 * The run keeps the device tables and outputs between calls (one call per launch of a driver
 * loop costs two kernel passes, one small round trip for the offsets and three copies).  k = 2
 * flip runs only (FC_ERR_UNSUPPORTED otherwise, ReCom runs with a move log included). */
int fc_run_frame_series_changes(fc_run *r, int32_t c0, int32_t nc, int32_t n_frame, const int32_t *frame_u,
                                const int32_t *frame_v, const double *mid_xy, double cx, double cy, int64_t cap,
                                int64_t *offsets, int64_t *t, double *slope, double *angle);
/* ---- election series: what the sampled plans do (gerrychain's Tally / Election updaters and the
 * seats / efficiency-gap outlier histograms), by a device replay of the event log against node
 * columns.  Flip runs, and ReCom runs with a move log (above), with FC_DIAG_SERIES; any k.
 * Over the window's yields t = series_t0 .. steps, with a_t the assignment at yield t:
 *   S_t[d][j]       = sum of node_cols[u][j] over the nodes u with a_t(u) = d;
 *   tally_now[d][j] = S at the current yield;      tally_sum[d][j] = sum_t S_t[d][j];
 * and per election e = (A, B) = (col_a[e], col_b[e]), with a_d = S_t[d][A], b_d = S_t[d][B]:
 *   A wins district d iff a_d > b_d (a tie is won by neither); seats_t = districts A wins;
 *   seats_hist[e][s] = yields with seats_t = s (s = 0..k); wins_sum[e][d] = yields in which A wins d;
 *   gap_t = sum_d g(a_d, b_d), g(a, b) = 3b - a if a > b, b - 3a if a < b, 0 on a tie: the
 *           efficiency gap (wasted_B - wasted_A) / total in units of 1 / (2 total votes),
 *           positive when it favours A (gerrychain's efficiency_gap is gap_t / (2 V));
 *   gap_sum[e] = sum_t gap_t;  gap_hist[e][i] = yields with i = the number of gap_edges <= gap_t
 *           (numpy searchsorted(gap_edges, gap_t, side="right")), i = 0..n_gap_edges.
 * All exact integers; every histogram row of a chain sums to its window's yields.
 *
 * fc_run_set_elections copies and uploads node_cols [n * n_cols] (1 <= n_cols <= 8; values >= 0,
 * every column total <= 2^31 - 1), the elections (0 <= n_elections <= 4: 0 keeps the tallies
 * only; col_a[e] != col_b[e], both below n_cols) and the strictly ascending gap_edges
 * (0 <= n_gap_edges <= 256; 0: no gap histogram).  Callable again to replace them.  The columns
 * are not trajectory state: checkpoint blobs do not hold them (and are byte for byte what they
 * were), so a restored run needs fc_run_set_elections again.
 * fc_run_election_series fills the outputs of chains [c0, c0 + nc) (any may be NULL to skip it)
 * and synchronises.  FC_ERR_ARG without FC_DIAG_SERIES, before fc_run_set_elections, for a bad
 * chain range, for gap_hist without edges, for a window of 2^30 yields or more, or when a chain's
 * log overflowed event_cap; FC_ERR_UNSUPPORTED for ReCom runs without a move log. */
int fc_run_set_elections(fc_run *r, int32_t n_cols, const int32_t *node_cols, int32_t n_elections,
                         const int32_t *col_a, const int32_t *col_b, int32_t n_gap_edges, const int64_t *gap_edges);
int fc_run_election_series(fc_run *r, int32_t c0, int32_t nc,
                           int64_t *tally_now, int64_t *tally_sum,  /* [nc * k * n_cols]                     */
                           int64_t *seats_hist,                      /* [nc * n_elections * (k + 1)]          */
                           int64_t *wins_sum,                        /* [nc * n_elections * k]                */
                           int64_t *gap_sum,                         /* [nc * n_elections]                    */
                           int64_t *gap_hist);                       /* [nc * n_elections * (n_gap_edges + 1)] */
/* The per-yield rule of one election, by the code the device runs: a, b [k] the districts'
 * tallies of the two columns (0 <= a, b <= 2^31 - 1, 1 <= k <= 32); *seats = districts A wins,
 * *gap = sum_d g(a_d, b_d).  Either output may be NULL.  Pure host function. */
int fc_election_eval(int32_t k, const int64_t *a, const int64_t *b, int32_t *seats, int64_t *gap);
/* ---- compactness series: how the sampled plans are shaped (gerrychain's perimeter,
 * exterior_boundaries, interior_boundaries and polsby_popper updaters), by a device replay of the
 * event log against node areas and boundary lengths.  Flip runs, and ReCom runs with
 * a move log (above), with FC_DIAG_SERIES; any k.  Inputs, per run, not trajectory state:
 *   node_area[n]  int32 >= 0, total <= 2^31 - 1;
 *   node_ext[n]   int32 >= 0: the length of the unit's boundary on the outside of the whole region
 *                 (gerrychain's node attribute boundary_perim); NULL: all 0;
 *   edge_len[E]   int32 >= 0, in the canonical edge order of fc_graph_edges: the length two
 *                 adjacent units share (gerrychain's edge attribute shared_perim);
 *                 sum node_ext + sum edge_len <= 2^31 - 1;
 *   pp_edges[n_pp_edges]  strictly ascending int64, 0 <= n_pp_edges <= 64; 0: no histograms.
 * Over the window's yields t = series_t0 .. steps, with a_t the assignment at yield t, for
 * district d:
 *   A_t[d] = sum of node_area[u] over the nodes u with a_t(u) = d;
 *   P_t[d] = sum of node_ext[u] over those nodes + sum of edge_len[e] over the edges e = (u, w)
 *            with a_t(u) != a_t(w) and d in {a_t(u), a_t(w)}: a cut edge counts once for each of
 *            its two districts;
 *   Q_t[d] = min(floor(2^20 A_t[d] / P_t[d]^2), 2^31 - 1), and 0 when P_t[d] = 0: the
 *            Polsby-Popper score is 4 pi Q / 2^20 (2^20 A < 2^51 and P^2 < 2^62: one unsigned
 *            64-bit division is exact; an edge q <= Q iff q P^2 <= 2^20 A for P > 0);
 *   Qmin_t = min over d < k of Q_t[d]: the plan's least compact district.
 * Outputs per chain, all int64:
 *   area_now[d], perim_now[d], pp_now[d] = A, P, Q at the current yield;
 *   perim_sum[d] = sum_t P_t[d];   pp_sum[d] = sum_t Q_t[d];   pp_min_sum = sum_t Qmin_t;
 *   pp_hist[d][i] = yields with i = the number of pp_edges <= Q_t[d] (numpy
 *            searchsorted(pp_edges, Q_t[d], side="right")), i = 0..n_pp_edges;
 *   pp_min_hist[i] = the same for Qmin_t.
 * All exact integers; every histogram row of a chain sums to its window's yields.
 *
 * fc_run_set_shapes validates and uploads the inputs (as per-node neighbour rows).  Callable
 * again to replace them.  Checkpoint blobs do not hold them (and are byte for byte what they
 * were), so a restored run needs fc_run_set_shapes again.  FC_ERR_ARG without FC_DIAG_SERIES, for
 * negative values or totals over 2^31 - 1, for edges that do not ascend or more than 64 of them;
 * FC_ERR_UNSUPPORTED for ReCom runs without a move log and when a chain's image (assignment,
 * histograms, a chunk's neighbour rows) does not fit 48 KB of LDS.
 * fc_run_shape_series fills the outputs of chains [c0, c0 + nc) (any may be NULL to skip it) and
 * synchronises.  FC_ERR_ARG without FC_DIAG_SERIES, before fc_run_set_shapes, for a bad chain
 * range, for a histogram without edges, for a window of 2^30 yields or more, or when a chain's log
 * overflowed event_cap; FC_ERR_UNSUPPORTED for ReCom runs without a move log. */
int fc_run_set_shapes(fc_run *r, const int32_t *node_area, const int32_t *node_ext, const int32_t *edge_len,
                      int32_t n_pp_edges, const int64_t *pp_edges);
int fc_run_shape_series(fc_run *r, int32_t c0, int32_t nc,
                        int64_t *area_now, int64_t *perim_now, int64_t *perim_sum, /* [nc * k]   */
                        int64_t *pp_now, int64_t *pp_sum,                          /* [nc * k]   */
                        int64_t *pp_min_sum,                                       /* [nc]       */
                        int64_t *pp_hist,      /* [nc * k * (n_pp_edges + 1)] */
                        int64_t *pp_min_hist); /* [nc * (n_pp_edges + 1)]     */
/* The score of one district, by the code the device runs: *q = Q(area, perim) as above.
 * FC_ERR_ARG for values below 0 or above 2^31 - 1.  Pure host function. */
int fc_shape_score(int64_t area, int64_t perim, int64_t *q);
/* ---- locality-splits series: how the sampled plans cut through administrative units
 * (gerrychain's county_splits updater and the split / pieces counts reported beside an ensemble),
 * by a device replay of the event log against a node labelling.  Flip runs, and ReCom
 * runs with a move log (above), with FC_DIAG_SERIES; any k.  Input, per run, not trajectory state:
 *   node_loc[n]  int32 labels in [0, n_loc), 1 <= n_loc <= n, every label used by at least one
 *                node.  One labelling per run; fc_run_set_localities is callable again to replace
 *                it (municipalities after counties: a second set + read over the same window).
 * Over the window's yields t = series_t0 .. steps, with a_t the assignment at yield t (it holds
 * from an event's t to the next event's):
 *   cells_t[c][d] = number of nodes u with node_loc[u] = c and a_t(u) = d;
 *   parts_t(c)    = number of d with cells_t[c][d] > 0 (at least 1);
 *   locality c is split iff parts_t(c) >= 2;   splits_t = number of split localities;
 *   excess_t      = sum_c (parts_t(c) - 1);
 *   sq_t          = sum_{c,d} cells_t[c][d]^2: the numerator of the Simpson-type preservation
 *                   index; divided by sum_c |c|^2 it is 1 when no locality is split;
 *   dlocs_t[d]    = number of localities district d meets;
 *   x_max         = sum_c min(|c|, k) - n_loc, the largest possible excess; X = min(x_max, 1023).
 * Outputs per chain, all int64:
 *   cells_now[c][d]  = cells at the current yield (parts, splits, excess, sq and dlocs "now"
 *                      follow from it on the host);
 *   split_sum[c]     = yields in which locality c is split;   parts_sum[c] = sum_t parts_t(c);
 *   dlocs_sum[d]     = sum_t dlocs_t[d];                      sq_sum = sum_t sq_t;
 *   splits_hist[s]   = yields with splits_t = s, s = 0..n_loc;
 *   excess_hist[x]   = yields with min(excess_t, X) = x, x = 0..X: the top bin collects every
 *                      larger excess.
 * All exact integers; both histogram rows sum to the window's yields.  FC_DIAG_SERIES limits n to
 * 65,535, so a cell fits 16 bits and sq_t < 2^32; with fewer than 2^30 window yields (checked)
 * nothing overflows int64.
 *
 * fc_run_set_localities validates and uploads the labels.  Checkpoint blobs do not hold them (and
 * are byte for byte what they were), so a restored run needs fc_run_set_localities again.
 * FC_ERR_ARG without FC_DIAG_SERIES, for n_loc < 1 or > n, a label out of range or an unused label;
 * FC_ERR_UNSUPPORTED for ReCom runs without a move log and when a chain's image does not fit 48 KB of
 * LDS: 8 (3 n_loc + X + 34) + 4 n_loc + 4 ceil(n_loc k / 2) + the assignment row (n padded to 16)
 * bytes; n <= 16,384 with n_loc <= 256 and n_loc k <= 4,096 always fits.
 * fc_run_split_series fills the outputs of chains [c0, c0 + nc) (any may be NULL to skip it) and
 * synchronises.  FC_ERR_ARG without FC_DIAG_SERIES, before fc_run_set_localities, for a bad chain
 * range, for a window of 2^30 yields or more, or when a chain's log overflowed event_cap;
 * FC_ERR_UNSUPPORTED for ReCom runs without a move log.  Calls interleave freely with the election, compactness and
 * frame series and with other chain ranges. */
int fc_run_set_localities(fc_run *r, int32_t n_loc, const int32_t *node_loc);
int fc_run_split_series(fc_run *r, int32_t c0, int32_t nc,
                        int64_t *cells_now,                      /* [nc * n_loc * k]  */
                        int64_t *split_sum, int64_t *parts_sum,  /* [nc * n_loc]      */
                        int64_t *dlocs_sum,                      /* [nc * k]          */
                        int64_t *sq_sum,                         /* [nc]              */
                        int64_t *splits_hist,                    /* [nc * (n_loc+1)]  */
                        int64_t *excess_hist);                   /* [nc * (X+1)]      */
/* The per-yield aggregates of one cell table, by the rule the device applies per flip (every
 * node entering its cell in turn): cells [n_loc * k], each 0 .. 65,535, every locality with at
 * least one node, n_loc >= 1, 1 <= k <= 32 (FC_ERR_ARG otherwise); *splits, *excess, *sq as
 * defined above.  Any output may be NULL.  Pure host function; its cost grows with the nodes. */
int fc_splits_eval(int32_t n_loc, int32_t k, const int64_t *cells,
                   int64_t *splits, int64_t *excess, int64_t *sq);
/* ---- plan samples: the ensemble itself, the assignments at thinned yields (the driver loop
 * "for i, part in enumerate(chain): if i % every == 0: save(part.assignment)"), by a device replay
 * of the event log up to chosen yields.  Flip runs, and ReCom runs with a move log
 * (above), with FC_DIAG_SERIES; any k; no
 * setter, nothing kept between calls.  Chain c has a series window of yields t = series_t0 .. steps;
 *   a_t = the window-start assignment with every logged event of t_e <= t applied in log order (an
 *         event's t is the first yield with a[v] = target).
 * The call takes one list times[0 .. n_times) of absolute yield indices, strictly increasing, the
 * same for every chain of the call, each inside every chain's window.  For sample j of chain
 * c0 + cl:
 *   plans[cl][j][u] = a_{times[j]}(u), the district index 0 .. k - 1 exactly as fc_run_read_state
 *                     reports it, rows packed to n bytes;
 *   cut[cl][j], nb[cl][j] = |cut| and |B| at that yield: the fields of the last event with
 *                     t_e <= times[j], and series_cut0 / series_nb0 when there is none;
 *   dist0[cl][j]    = the number of nodes u with a_{times[j]}(u) != a_{series_t0}(u), the Hamming
 *                     distance to the window-start plan;
 *   pops[cl][j][d]  = the sum of pop[u] over the nodes with a_{times[j]}(u) = d.
 * All exact integers; plans is int8, the others int64.  The row of a sample at times[j] = steps is
 * what fc_run_read_state and fc_run_read_pops return, and a sample at series_t0 is the window-start
 * plan with dist0 = 0.  Several samples between two events repeat the same plan.
 *
 * Any output may be NULL to skip it (without plans no row is staged); the call synchronises; nc = 0
 * or n_times = 0 is FC_OK and writes nothing.  FC_ERR_ARG without FC_DIAG_SERIES, for a bad chain
 * range, n_times < 0, NULL times with n_times > 0, times not strictly increasing, a time before a
 * chain's series_t0 or after its steps (the message names the chain and the time), a chain whose
 * log overflowed event_cap, or when the staged rows (nc * n_times * npad bytes, npad = n rounded up
 * to 16) exceed a tenth of the free device memory: split the call by chains or by times.
 * FC_ERR_UNSUPPORTED for ReCom runs without a move log.  Every n a run admits is supported: a chain's
 * image is npad + 256 bytes of LDS, and there is no LDS refusal.  Calls interleave freely with the other series calls and with other chain ranges;
 * checkpoint blobs are byte for byte what they were, and a restored run can be sampled at once. */
int fc_run_sample_plans(fc_run *r, int32_t c0, int32_t nc, int32_t n_times, const int64_t *times,
                        int8_t *plans,                               /* [nc * n_times * n] */
                        int64_t *cut, int64_t *nb, int64_t *dist0,   /* [nc * n_times]     */
                        int64_t *pops);                              /* [nc * n_times * k] */
/* Device time of the last fc_run_sample_plans call that launched (HIP events on the run's stream):
 * the kernel, and the copy of the plan rows to the host (0 when plans was NULL).  Either may be
 * NULL.  FC_ERR_ARG before the first such call. */
int fc_run_sample_plans_ms(fc_run *r, float *kernel_ms, float *copy_ms);
/* ---- heat-map series: the reference's main outputs (per-edge cut_times :383-384, per-node flip
 * counts and label integrals :396-400, the histograms of len(cut_edges) and len(b_nodes)) over the
 * series window, by a device replay of the event log.  Flip runs of any k, and
 * ReCom runs with a move log (above), with FC_DIAG_SERIES; no setter, nothing kept between calls
 * (the run keeps the neighbour / edge rows it builds on the first call).  The window's yields are
 * t = series_t0 .. steps, both inclusive;
 *   a_t = the window-start assignment with every logged event of t_e <= t applied in log order.
 * Per chain, edges in fc_graph_edges order, all exact int64:
 *   cut_hist[x]   = yields with |cut| = x, x = 0..E;   nb_hist[x] = the same for |B|,
 *                   x = 0..fc_run_nb_width - 1.  |cut| and |B| at yield t are those of the last
 *                   event with t_e <= t, and series_cut0 / series_nb0 when there is none; each row
 *                   sums to the window's yields;
 *   cut_times[e]  = yields with a_t(eu[e]) != a_t(ev[e]);
 *   moves[u]      = logged events on u: the accepted flips of u (flip runs), the accepted steps
 *                   that moved u (ReCom runs); either way the yields t of the window with
 *                   a_t(u) != a_{t-1}(u);
 *   last_move[u]  = t of the last event on u, 0 when there is none (last_accept's convention;
 *                   events have t >= 1);
 *   dwell[u][d]   = yields with a_t(u) = d; every node's row sums to the window's yields.
 * Over a window from yield 0 of a flip run, cut_hist / nb_hist are fc_run_read_hist's rows,
 * cut_times fc_run_read_edges', moves and last_move fc_run_read_flips_exact's flip_count and
 * last_accept, and sum_d labels[d] dwell[u][d] its occupancy; ReCom runs have no other source
 * of them.
 *
 * Any output may be NULL to skip it; nc = 0 is FC_OK and writes nothing; the call synchronises.
 * The replay accumulates in the output rows in device memory (the global-rows form, the default: a
 * chain's workgroup then needs little LDS and many chains share a compute unit, which measured 4.7
 * times faster on the C2 shape).  Under FC_HEAT_LDS_ROWS it keeps every requested
 * array of a chain in LDS beside its assignment and writes them out once at the end (the LDS form),
 * when that image fits the device's opt-in dynamic LDS limit (queried); an image that does not fit
 * takes the global-rows form all the same.  Same output either way.  There is no LDS refusal: every
 * n a logged run admits is supported.  FC_ERR_ARG without FC_DIAG_SERIES, for a bad chain
 * range, unknown flags, a window of 2^30 yields or more, a chain whose log overflowed event_cap
 * (the message names the chain), or when the requested outputs exceed a tenth of the free device
 * memory: split the call by chains.  FC_ERR_UNSUPPORTED for ReCom runs without a move log.  Calls
 * interleave freely with the other series calls and with other chain ranges; checkpoint blobs are
 * byte for byte what they were. */
#define FC_HEAT_LDS_ROWS 0x1u    /* privatise the requested arrays in LDS when the chain's image fits,
                                    instead of accumulating in the output rows in device memory
                                    (test / measurement knob: the slower form as measured)        */
int fc_run_heat_series(fc_run *r, int32_t c0, int32_t nc, uint32_t flags,
                       int64_t *cut_hist,    /* [nc * (E + 1)]                       */
                       int64_t *nb_hist,     /* [nc * nb_width]  (fc_run_nb_width)   */
                       int64_t *cut_times,   /* [nc * E]                             */
                       int64_t *moves,       /* [nc * n]                             */
                       int64_t *last_move,   /* [nc * n]                             */
                       int64_t *dwell);      /* [nc * n * k]                         */
/* The last fc_run_heat_series call that launched: *form = 0 the LDS form, 1 the global-rows form;
 * *lds_bytes = the dynamic LDS of one of its workgroups; *kernel_ms = the kernel's device time
 * (HIP events on the run's stream).  Any may be NULL.  FC_ERR_ARG before the first such call. */
int fc_run_heat_series_info(fc_run *r, int32_t *form, int64_t *lds_bytes, float *kernel_ms);
/* The neighbour / edge rows the heat-map replay walks, by the code that builds them: *width = slots
 * per row (8 or 16); nbr / eid [n * width]: slot j of node u holds a neighbour and the canonical id
 * (fc_graph_edges order) of the edge to it, -1 / -1 when empty.  nbr and eid may be NULL (width
 * only).  Pure host function; FC_ERR_UNSUPPORTED for a node degree above 16. */
int fc_graph_heat_rows(const fc_graph *g, int32_t *width, int32_t *nbr, int32_t *eid);
/* ---- short bursts: the score of every yield of the series window, the best of them, and the
 * restart of a ReCom chain from the plan it held there (gerrychain's
 * SingleMetricOptimizer.short_bursts: run b steps, keep the best plan the burst visited, ties to
 * the latest, restart from it), by a device replay of the event log.
 * A metric maps the state at one yield to an int64 score; a_d, b_d are district d's tallies of the
 * vote columns col_a, col_b of fc_run_set_elections:
 *   FC_BURST_COUNT  the districts with den * a_d > num * (a_d + b_d): with num / den = 1 / 2 the
 *                   seats of A exactly as fc_election_eval counts them (a tie is no win), with
 *                   another fraction the districts above a share; equality is not counted;
 *   FC_BURST_GAP    |sum_d g(a_d, b_d)|, g as in the election series, in its doubled integer units;
 *   FC_BURST_CUT    |cut| of the yield, from the event fields: it needs no columns.
 * maximize = 1 looks for the largest score, 0 for the smallest.  The best yield of a window
 * series_t0 .. steps is the LATEST yield whose score is best; the window-start state is a candidate,
 * and a yield made by a rejected step (no event) is a yield of the state before it, so a chain
 * whose last state has the best score has best_t = steps.                                         */
#define FC_BURST_COUNT 0
#define FC_BURST_GAP 1
#define FC_BURST_CUT 2
typedef struct fc_burst_metric {
    uint32_t struct_size;      /* sizeof(fc_burst_metric) as the caller compiled it (fc_burst_metric_init) */
    int32_t kind;              /* FC_BURST_*                                                */
    int32_t col_a, col_b;      /* vote kinds: two different columns of fc_run_set_elections */
    int64_t num, den;          /* FC_BURST_COUNT's share, 0 < num < den <= 2^20             */
    int32_t maximize;          /* 1: the largest score is best, 0: the smallest             */
} fc_burst_metric;
/* Zeroes *m and sets struct_size, kind = FC_BURST_CUT, num / den = 1 / 2, maximize = 1. */
int fc_burst_metric_init(fc_burst_metric *m, uint32_t struct_size);
/* The score of one state by the rule the device applies: a, b [k] the districts' tallies of the
 * metric's two columns (vote kinds; may be NULL for FC_BURST_CUT), cut its |cut|.  FC_ERR_ARG for
 * an unknown kind, num / den outside 0 < num < den <= 2^20, maximize other than 0 / 1, k outside
 * 1..32, a negative tally or cut, or den * (the sum of all the tallies) at 2^62 or above (a product
 * could overflow).  The columns are not read.  Pure host function. */
int fc_burst_eval(const fc_burst_metric *m, int32_t k, const int64_t *a, const int64_t *b, int64_t cut,
                  int64_t *score);
/* Scores every yield of the window of chains c0 .. c0 + nc - 1.  Per chain of the call, all int64:
 *   best_score, best_t     the best score and the absolute index of the latest yield that has it;
 *   start_score, end_score the scores at series_t0 and at steps;
 *   best_cut, best_nb      |cut| and |B| at best_t;
 *   best_plan [nc * n]     the assignment at best_t (int8, as fc_run_read_state reports it).
 * Any output may be NULL.  Without flags nothing in the run changes: flip runs of any k and ReCom
 * runs with a move log, with FC_DIAG_SERIES.  With FC_BURST_REWIND (ReCom runs only:
 * FC_ERR_UNSUPPORTED for a flip run, whose derived per-node state a rewind would have to rebuild)
 * every chain of the range restarts from its best plan, written by the kernel on the device:
 * its assignment := the plan at best_t, its cut / nb := those of best_t, and its series window
 * restarts there exactly as fc_run_series_reset leaves it (events = 0, series_t0 = steps,
 * series_cut0 / series_nb0 = cut / nb, window-start plan = the plan).  draws, steps, every counter
 * and sum, and every chain outside the range are untouched: the draw counter continues, so a chain
 * whose best is its start plan does not repeat its burst, and the streaming sums (sum_cut, ...)
 * cover the abandoned yields too.
 * Checked before any device work (a refused call changes nothing): FC_ERR_ARG for a bad metric
 * (as fc_burst_eval; columns >= n_cols or equal; den * the two columns' totals at 2^62 or above),
 * unknown flags, a vote kind before fc_run_set_elections, a bad chain range, a window of 2^30
 * yields or more, a chain whose log overflowed event_cap; FC_ERR_UNSUPPORTED for ReCom runs
 * without a move log and for a chain image (n rounded up to 16, + 256 bytes) above 48 KB of LDS. */
#define FC_BURST_REWIND 0x1u     /* restart every chain of the range from its best plan (ReCom runs) */
int fc_run_burst_select(fc_run *r, int32_t c0, int32_t nc, const fc_burst_metric *metric, uint32_t flags,
                        int64_t *best_score, int64_t *best_t, int64_t *start_score, int64_t *end_score,
                        int64_t *best_cut, int64_t *best_nb,       /* [nc] each  */
                        int8_t *best_plan);                        /* [nc * n]   */
/* Device time of the last fc_run_burst_select call's kernel (HIP events on the run's stream).
 * FC_ERR_ARG before the first such call. */
int fc_run_burst_select_ms(fc_run *r, float *kernel_ms);
/* Page-lock (pin) a caller's host buffer for faster device-to-host copies of the readers above
 * (hipHostRegister); unregister before freeing it. */
int fc_host_register(void *ptr, int64_t bytes);
int fc_host_unregister(void *ptr);
/* ---- checkpoint / resume ---------------------------------------------------- */
/* Everything later fc_run_steps calls depend on -- every chain's assignment, foreign-neighbour
 * counts, draw counter, counters and sums, populations, acceptance thresholds, district-graph
 * tables, and the enabled per-yield accumulators (histograms, cut_times, flips, the series
 * window and event log) -- as one byte blob.  fc_run_checkpoint with buf == NULL (or cap too
 * small) stores the size in *len (FC_ERR_ARG when cap is too small).  fc_run_restore loads it
 * into a run created with the same graph and fc_params (n_chains, k, proposal, diag_mask,
 * event_cap, seed, chain_id_offset and a hash of every trajectory-determining parameter --
 * per-chain bases / thresholds and population bounds, labels, the log(1 - p) table, accept /
 * constraint settings, frozen nodes, ReCom settings -- are checked; FC_ERR_ARG otherwise); the
 * chains then continue bit for bit as if never interrupted.  Per-proposal traces are outputs: they restart empty after a restore. */
int fc_run_checkpoint(fc_run *r, void *buf, int64_t cap, int64_t *len);
int fc_run_restore(fc_run *r, const void *buf, int64_t len);
/* ---- replica exchange (parallel tempering) between chains of one run ---------------------- */
/* No reference counterpart: the reference runs one chain per (base, tolerance) and shows that it
 * mixes torpidly away from base 1; this is the standard remedy, defined here (DESIGN.md "Replica
 * exchange").  A ladder is an ordered list of local chain indices, rung 0 first; a chain is in at
 * most one ladder and chains in none are never touched.  Replicas keep their state, draw counter
 * and accumulators; what moves between the chains of a ladder is the temperature (the base, i.e.
 * the chain's acceptance thresholds).  Replica x at rung r (base b_r) and y at rung r + 1 swap
 * with probability min(1, (b_r / b_{r+1}) ** (|cut_x| - |cut_y|)), which preserves the product of
 * the rungs' stationary laws.  The uniform of the pair with lower rung r in round t is
 * mant53(x0, x1) of Philox4x32-10(ctr = (t, r, G, 4), key = seed), G the global id
 * (chain_id_offset + index) of the ladder's first-listed chain: no dependence on the sharding.
 *
 * fc_run_set_ladders: ladder l lists members[ladder_off[l] .. ladder_off[l + 1] - 1]
 * (ladder_off[0] = 0); "slot" ladder_off[l] + r below is rung r of ladder l.  Callable once,
 * before or between launches (what a chain accumulated before counts for its initial rung).
 * FC_ERR_UNSUPPORTED for ReCom runs and accept kinds other than FC_ACCEPT_CUT (and graphs with
 * 2^17 or more edges); FC_ERR_ARG for an index out of range, a chain listed twice, members of one
 * ladder with different population bounds (bounds are never swapped), a non-positive base,
 * unknown flags, FC_LADDER_HIST without FC_DIAG_HIST, or a second call; FC_ERR_NOMEM when the
 * FC_LADDER_HIST buffers (a snapshot of both histograms and one row pair per slot) do not fit. */
#define FC_LADDER_HIST 0x1u      /* keep the |cut| and |B| histograms per rung as well           */
int fc_run_set_ladders(fc_run *r, int32_t n_ladders, const int32_t *ladder_off, const int32_t *members,
                       uint32_t flags);
/* One exchange round, asynchronous on hip_stream (NULL = the run's stream; use the stream of the
 * fc_run_steps calls it separates): every ladder chain's sums since the last round are attributed
 * to the rung it held, then the pairs (r, r + 1) with r = parity (mod 2) are tried; parity -1
 * means (round counter & 1).  The round counter starts at 0 and advances by one per call.
 * FC_ERR_ARG without ladders or for another parity. */
int fc_run_exchange(fc_run *r, int32_t parity, void *hip_stream);
/* rung_of [n_chains]: the rung each chain holds now (-1: in no ladder); chain_at [members]: the
 * chain at each slot.  Either may be NULL.  Synchronises. */
int fc_run_read_rungs(fc_run *r, int32_t *rung_of, int32_t *chain_at);
/* bases [n_chains]: the base each chain runs at now (also valid without ladders). */
int fc_run_read_bases(fc_run *r, double *bases);
/* Per-slot (per-temperature) statistics: the streaming sums of whichever replicas held the slot,
 * each launch's deltas going to the rung held during it (the initial yield to the initial rung),
 * and the swaps tried / accepted of the pair (slot, slot + 1). */
typedef struct fc_rung_stats {
    int64_t steps, proposals, draws, accepted, inv_contig, inv_pop;
    int64_t sum_cut, sum_nb, sum_wait, sum_cut2, sum_nb2;   /* as in fc_chain_stats              */
    int64_t swaps_tried, swaps_accepted;                    /* pair (this slot, next slot)       */
} fc_rung_stats;
/* Attributes what is outstanding (no swap, no round counted), then copies: out [members];
 * cut_hist [members * (E + 1)] and nb_hist [members * fc_run_nb_width] with FC_LADDER_HIST (NULL
 * to skip; FC_ERR_ARG when asked for without it). */
int fc_run_read_rung_stats(fc_run *r, fc_rung_stats *out, int64_t *cut_hist, int64_t *nb_hist);
/* The U53 threshold of one swap decision, by the code the device runs: the pair of rungs with
 * bases (b_lo_rung, b_hi_rung) and d = |cut| of the lower rung's replica - |cut| of the upper's
 * swaps iff mant53 < *t.  2^53 when (b_lo_rung / b_hi_rung) ** d >= 1; otherwise
 * ceil(p 2^53), p the product over the set bits j of |d| (ascending) of pow(qq, 2^j),
 * qq = min(b) / max(b), cut to 0 once below 2^-64.  Pure host function; |d| < 2^17. */
int fc_ladder_swap_threshold(double b_lo_rung, double b_hi_rung, int32_t d, uint64_t *t);
/* Checkpoints of a run with ladders append the rung map, the snapshots, the per-slot sums and
 * histograms, the swap counters and the round counter, and carry a hash of the ladder layout; they
 * restore only into a run with the same ladders set (FC_ERR_ARG otherwise, also for a run
 * without ladders).  Blobs of runs without ladders are unchanged. */
/* Name of the last launched flip-kernel instance, as rocprofv3 spells it. */
int fc_run_kernel_name(const fc_run *r, char *buf, int32_t cap);
int32_t fc_run_n_chains(const fc_run *r);
/* LDS bytes one chain's state takes on the device (one chain per wavefront; the chains a CU
 * holds at once is 160 KiB / this, or the VGPR limit) -- for sizing launches to one wave of
 * resident chains. */
int32_t fc_run_chain_lds_bytes(const fc_run *r);
/* Entries of a chain's |B| histogram row and of the log1mp table: n + 1, or with
 * FC_FLAG_NB_PAIRS (k > 2) sum_u min(deg u, k - 1) + 1, the largest pair count + 1. */
int32_t fc_run_nb_width(const fc_run *r);
/* Which paths the memory-dependent diagnostics took (outputs are the same either way):
 * the k = 2 tally log's entries per chain granted (*tally_log_cap; 0 = none, every tally by
 * global atomics) against those the last launch asked for (*tally_log_wanted: a granted size
 * below it means chains may have filled the log and applied the rest by atomics), and whether
 * the last fc_run_frame_series_changes ran one staged pass (*series_staged = 1), the two-pass
 * form (0) or none yet (-1). */
int fc_run_diag_paths(const fc_run *r, int64_t *tally_log_cap, int64_t *tally_log_wanted, int32_t *series_staged);
/* The ring-verdict table of a k = 2 flip run on rings of at most 8 cells (fc_params.tune_ring_table):
 * the classes the graph's rings fall into (*classes; 0 for any other run) and whether the run holds
 * a table (*in_use = 1) or none (0: more classes than the cap, the knob at 0, or a node with more
 * than four neighbours).  A table is read by the launches of the lean node-stream instance
 * (fc_run_kernel_name: flip2_kernel<8, *, false, false, false, false>); a run with diagnostics, the
 * band stream or the search holds it unread and evaluates the arithmetic.  The verdicts are the
 * same either way. */
int fc_run_ring_table(const fc_run *r, int32_t *classes, int32_t *in_use);
/* The pass plan of the run's last k = 2 tally reduce (the tally counterpart of fc_run_kernel_name):
 * the device's dynamic-LDS limit it was planned for (*lds_limit), the number of passes (*n_passes;
 * 0: no reduce has run; at most 9) and, for the first min(*n_passes, cap) of them, the arrays each
 * kept in LDS (lds_masks[i], bit a = array a in the order cut_hist, nb_hist, cut_times, num_flips,
 * part_sum, last_flipped, flip_count, occupancy, last_accept) and the LDS bytes it asked for
 * (lds_bytes[i]); *global_mask: the arrays applied with global atomics -- those above the limit
 * and those of a pass the device refused (that pass then reads mask 0, 0 bytes). */
int fc_run_tally_plan(const fc_run *r, int64_t *lds_limit, int32_t *n_passes, uint32_t *lds_masks, int64_t *lds_bytes,
                      int32_t cap, uint32_t *global_mask);
void fc_run_destroy(fc_run *r);

int fc_device_count(int32_t *n);
/* PCI bus id ("dddd:bb:dd.f") of HIP device `device` (hipDeviceGetPCIBusId): an N-GPU bench line
 * lists every rank's, so it shows that N distinct GPUs did the work. */
int fc_device_pci_id(int32_t device, char *buf, int32_t cap);
const char *fc_last_error(void);

/* What this library was built with (FC_BUILD_* bits; 0 = the product build).  A profiling or
 * experiment build counts phases in the kernels or was compiled with extra flags: its timings
 * are not the product's, so the Python loader refuses it unless asked (_lib.load(allow_variant)). */
#define FC_BUILD_PHASE_PROF 0x1u   /* -DFC_PHASE_PROF: per-phase s_memtime counters per chain   */
#define FC_BUILD_PHASE_SYNC 0x2u   /* -DFC_PHASE_SYNC: each stamp drains outstanding memory     */
#define FC_BUILD_VARIANT 0x4u      /* built with FC_LIB_VARIANT / FC_HIPCC_FLAGS (tools only)   */
uint32_t fc_build_flags(void);
/* Identity of the sources this library was compiled from: the hex SHA-256 of every source and
 * header plus the compiler flags, passed in by the build (flipcomplexityempirical_amd/build.py).
 * The in-tree loader rebuilds when it differs from the current sources' id (never by file
 * times), and profiles record it so counters are matched to the kernel revision they measured. */
const char *fc_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
