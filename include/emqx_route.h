/*
 * emqx_route.h — C ABI of the route table and the batched route stage (libemqxmatch.so): the
 * step of emqx_broker:publish/1 between emqx_router:match_routes/1 and dispatch.
 *
 * The match engine answers {F : emqx_topic:match(T, F)} as a CSR of filter ids.  match_routes/1
 * itself returns #route{topic, dest} records, and its caller is
 *
 *   route(aggre(emqx_router:match_routes(Topic)), delivery(Msg))   apps/emqx/src/emqx_broker.erl:213
 *
 * Paths are relative to the reference checkout (xiongzhenhai-zh/emqx, EMQX 5.0.0-beta.3):
 *
 *   the route table, a bag of #route{topic, dest}   apps/emqx/src/emqx_router.erl:75-83
 *     dest = Node | {Group, Node}; replicated to every node (:135)
 *   do_add_route/2 (idempotent)                     emqx_router.erl:111-124
 *   do_delete_route/2                               emqx_router.erl:163-171
 *   lookup_routes/1                                 emqx_router.erl:142-144
 *   match_routes/1                                  emqx_router.erl:127-133
 *   cleanup_routes/1 (a node went down)             apps/emqx/src/emqx_router_helper.erl:171-175
 *   aggre/1                                         emqx_broker.erl:261-272
 *     plain routes stay one each; {To, Group} collapses over the nodes that host members of the
 *     group (the lists:usort at :271)
 *   route/2, do_route/2                             emqx_broker.erl:244-259
 *     {To, Node} when Node =:= node()  -> dispatch(To, Delivery)            (LOCAL)
 *     {To, Node}                       -> forward(Node, To, Delivery, Mode) (REMOTE), :277-279
 *     {To, Group}                      -> emqx_shared_sub:dispatch/3        (SHARE)
 *     route([], _): 'message.dropped' with no_subscribers (:244-247)
 *
 * This stage holds the bag in device memory, dense by filter id, and turns a batch's match CSR
 * into: a flags byte per entry, the length of aggre(match_routes(T_i)) per message, one forward
 * list per node, and the CSR of the entries this node dispatches itself (what a cluster node
 * feeds to emqx_fanout_batch_device_async instead of the full match CSR).
 *
 * Left to the caller: the RPC itself and its sync or async mode; the {Node, To, Result} result
 * tuples; the maps from node and group names to ids; which subscriber a group picks (the
 * fan-out's job: its subscriber table already holds the members of every node);
 * emqx_session_router's session-id dests.
 *
 * Conventions as in emqx_match.h and emqx_select.h: int status, EMQX_* codes.  One writer (add /
 * remove / purge / commit) at a time; any number of concurrent route callers read the
 * committed, immutable snapshot.
 */
#ifndef EMQX_ROUTE_H
#define EMQX_ROUTE_H

#include <stdint.h>

#include "emqx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emqx_routetab emqx_routetab;

#define EMQX_ROUTE_HOST_ONLY (-2)        /* `device` of a handle without a device               */
#define EMQX_ROUTE_MAX_NODES 64          /* node ids are 0..63: one mask bit per node, one lane
                                            of a wave per node; above any EMQX cluster in use  */
#define EMQX_ROUTE_MAX_FILTER (1u << 30) /* filter ids are below this, as everywhere            */

/* entry_flags[d]; 0: the table does not know the id or it has no dest (ids >= 2^30 and
 * 0xFFFFFFFF included). */
#define EMQX_ROUTE_LOCAL 0x1u  /* a plain route to local_node: dispatch(To) runs here           */
#define EMQX_ROUTE_SHARE 0x2u  /* >= 1 grouped dest: emqx_shared_sub:dispatch/3 once per group  */
#define EMQX_ROUTE_REMOTE 0x4u /* >= 1 plain route to another node                              */

/* summary[8]: [0] flags, [1] CSR entries read, [2] forwards, [3] messages with msg_routes = 0
 * (route([], _): dropped, no_subscribers), [4] messages with at least one forward, [5] entries
 * kept in the local CSR, [6] entries with flags 0, [7] nodes with at least one forward. */
#define EMQX_ROUTE_SUMMARY_WORDS 8
#define EMQX_ROUTE_F_FWD_OVERFLOW 0x1u  /* forwards > cap_fwd: node_offsets complete, fwd_* untouched       */
#define EMQX_ROUTE_F_INPUT_REFUSED 0x2u /* offsets[n] > cap_in: nothing read or written but the summary     */

/* One route call.  Every pointer is host memory for emqx_route_batch (the function) and
 * emqx_route_host, device memory for the _device forms.  Every output is a pure function of the
 * input: two runs are byte-identical.
 *
 * In:  the match CSR as emqx_match_batch_device* writes it in EMQX_MODE_ROUTES: offsets[n+1]
 *      with offsets[0] = 0, filters[] of capacity cap_in.  n < 2^32.
 *      AN ENTRY IS TREATED ON ITS OWN: a filter id that occurs twice in a message forwards
 *      twice and counts twice.  The engine never emits that.
 * Out: entry_flags[cap_in] (may be NULL): EMQX_ROUTE_* of each entry.
 *      msg_routes[n]: the length of aggre(match_routes(T_i)): over the message's entries, the
 *        filter's plain routes plus its distinct groups.
 *      node_offsets[EMQX_ROUTE_MAX_NODES + 1], fwd_msgs[cap_fwd], fwd_filters[cap_fwd]: node v's
 *        extent [node_offsets[v], node_offsets[v+1]) holds one (message, filter) per entry whose
 *        filter has a plain route to v, v != local_node, in ascending entry position (message
 *        order, CSR order within a message).  The local node's extent is empty.
 *      local_offsets[n+1], local_filters[cap_in] (both or neither): the entries with LOCAL or
 *        SHARE, per message in input order. */
struct emqx_route_batch {
  const uint64_t* offsets;
  const uint32_t* filters;
  uint64_t n;
  uint64_t cap_in;
  uint8_t* entry_flags;
  uint32_t* msg_routes;
  uint64_t* node_offsets;
  uint32_t* fwd_msgs;
  uint32_t* fwd_filters;
  uint64_t cap_fwd;
  uint64_t* local_offsets;
  uint32_t* local_filters;
};

/* Versioned by size, as emqx_stats: set `size` = sizeof(emqx_routetab_stats) before the call. */
typedef struct emqx_routetab_stats {
  uint64_t size;        /* in: sizeof(emqx_routetab_stats) of the caller; out: bytes written */
  uint64_t n_filters;   /* filter ids with at least one dest, committed snapshot             */
  uint64_t n_plain;     /* plain routes #route{dest = Node}                                   */
  uint64_t n_grouped;   /* grouped routes #route{dest = {Group, Node}}                        */
  uint64_t n_nodes;     /* nodes that occur in a dest                                         */
  uint64_t epoch;       /* commits so far                                                     */
  double last_build_ms; /* host build + upload time of the last commit                        */
  double last_call_ms;  /* time of the last synchronous route call                            */
} emqx_routetab_stats;

/* device >= 0: a HIP device (-1: the current one).  EMQX_ROUTE_HOST_ONLY: a handle that takes
 * changes, commits and answers emqx_route_host; its batch entry points return EMQX_EDEVICE
 * (nothing ever falls back to the host silently).  local_node >= EMQX_ROUTE_MAX_NODES:
 * EMQX_EINVAL. */
int emqx_routetab_create(int32_t device, uint32_t local_node, emqx_routetab** out);
int emqx_routetab_destroy(emqx_routetab* h);

/* do_add_route/2 for n dests (filter_ids[i], nodes[i], groups[i]); groups NULL or
 * groups[i] = EMQX_NO_GROUP: the plain route #route{dest = Node}, else {Group, Node}.  A triple
 * occurs at most once: adding it again changes nothing.  EMQX_EINVAL, nothing changed: a filter
 * id >= 2^30, a node >= EMQX_ROUTE_MAX_NODES. */
int emqx_routetab_add(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups,
                      uint64_t n);
/* do_delete_route/2, same arguments; absent triples are ignored. */
int emqx_routetab_remove(emqx_routetab* h, const uint32_t* filter_ids, const uint32_t* nodes, const uint32_t* groups,
                         uint64_t n);
/* cleanup_routes/1: removes every dest on `node`, plain and grouped, and reports in
 * emptied[0, cap) the filter ids left without any dest, ascending (the caller deletes them from
 * the engine as delete_trie_route would).  *n_emptied (may be NULL) = their number; when it
 * exceeds cap: EMQX_EOVERFLOW and NOTHING IS REMOVED. */
int emqx_routetab_purge_node(emqx_routetab* h, uint32_t node, uint32_t* emptied, uint64_t cap, uint64_t* n_emptied);
/* lookup_routes/1 from the host image (commit or not), in insertion order: nodes_out[k],
 * groups_out[k] (EMQX_NO_GROUP: plain).  *n (may be NULL) = the dests of the filter; more than
 * cap: EMQX_EOVERFLOW, the first cap written. */
int emqx_routetab_lookup(emqx_routetab* h, uint32_t filter_id, uint32_t* nodes_out, uint32_t* groups_out, uint64_t cap,
                         uint64_t* n);
/* Builds the device records of every filter (16 bytes each, dense by filter id), uploads them
 * with one copy and swaps them in.  Calls in flight keep the snapshot they started on; changes
 * are invisible to route calls until a commit. */
int emqx_routetab_commit(emqx_routetab* h);

/* Host buffers, evaluated on the device.  EMQX_EINVAL: offsets[0] != 0, decreasing offsets,
 * offsets[n] > cap_in.  *n_fwd (may be NULL) = the forwards; when they exceed cap_fwd:
 * EMQX_EOVERFLOW, *n_fwd = the capacity needed, node_offsets and every other output complete,
 * fwd_msgs and fwd_filters untouched.  summary_out (host, may be NULL): the 8 summary words. */
int emqx_route_batch(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out);
/* Device buffers, on `stream` (NULL: the table's own, ordered after the device's null stream);
 * synchronizes the stream.  The entry count is read on the device.  Returns as above;
 * offsets[n] > cap_in: EMQX_EINVAL with summary flag bit 1. */
int emqx_route_batch_device(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out,
                            void* stream);
/* Enqueues the call on `stream` and returns at once: the form that chains behind
 * emqx_match_batch_device_async on the same stream.  `summary` (>= 8 uint64_t, device or
 * host-pinned memory) is written when the stream reaches it.  Whatever the device buffers hold,
 * no access leaves them.  The snapshot the call reads stays alive until the call has drained. */
int emqx_route_batch_device_async(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* summary, void* stream);
/* The same bytes computed on the calling thread over the same committed snapshot, with the same
 * per-record code the kernels run: the per-call path and the checker of the batch path. */
int emqx_route_host(emqx_routetab* h, const struct emqx_route_batch* b, uint64_t* n_fwd, uint64_t* summary_out);

/* Keys: "max_blocks" (1..16384, default 16384): the grid cap of the by-tile passes, the blocks
 * stride over the tiles beyond it; "scan_chunk" (1..1024, default 1024): the elements the one-block
 * scans take per carry step (tests lower both to make the blocks stride and the scans carry at
 * small shapes; the same bytes at every value); "path" (0: ballot ranks, the default; 1: expand, library
 * radix sort, gather: the yardstick; both write the same bytes); "stored_mask" (1, the default: the
 * second by-tile pass reads a word the first stored per entry, 8 bytes of scratch per entry of
 * cap_in; 0: it gathers the records again; the same bytes either way).  EMQX_ENOTFOUND for unknown keys. */
int emqx_routetab_set_tuning(emqx_routetab* h, const char* key, int64_t value);
int emqx_routetab_stats_get(emqx_routetab* h, emqx_routetab_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* EMQX_ROUTE_H */
