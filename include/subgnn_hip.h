/*
 * subgnn_hip.h -- C ABI of libsubgnn_hip.so: the MI355X (gfx950) kernels behind SubGNN's
 * anchor-patch sampling + three-channel subgraph message-passing hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (torch tensors on the host
 *     side); nothing is allocated or freed inside; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*), graph-capturable, and stateless: the library keeps no settings between
 *     calls (where two kernels compute the same values, the choice is an argument of the call: `kernel`, `pull_alpha`);
 *   - return value: 0 = launched, negative = SGNN_ERR_* (argument errors are detected on the
 *     host before any launch; nothing throws across the ABI);
 *   - node ids are 1-based, 0 = PAD (reference config.py:9, SubGNN/SubGNN.py:554-559);
 *   - the base graph is CSR indexed by node id: rowptr int64[max_id + 2] (row 0 = PAD, empty),
 *     col int32[nnz]; `col` keeps networkx neighbour order (needed by the walks),
 *     `col_sorted` is the same rows sorted ascending (adjacency tests by binary search);
 *   - ragged sets (connected components, anchor patches, subgraphs) are
 *     set_ptr int64[n_sets + 1] + set_nodes int32[set_ptr[n_sets]], PAD already stripped,
 *     order preserved, duplicates kept -- never the reference's dense zero padding;
 *   - randomness is the counter-based draw tape draw64(seed, stream, item, j) (DESIGN.md,
 *     "Draw tape"; oracle twin: oracle/tape.py).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference root, mims-harvard/SubGNN).
 */
#ifndef SUBGNN_HIP_H
#define SUBGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGNN_OK                  0
#define SGNN_ERR_BAD_ARG        -1
#define SGNN_ERR_SET_TOO_LARGE  -2   /* a set exceeds the size class a kernel supports */
#define SGNN_ERR_NNZ_TOO_LARGE  -3   /* nnz >= 2^31 (kernels index col with 32 bits) */
#define SGNN_ERR_LAUNCH         -4   /* hipGetLastError() after a launch */
#define SGNN_ERR_UNSUPPORTED_D  -5   /* embedding width not supported by the vector path */

#define SGNN_ABI_VERSION 14
int sgnn_abi_version(void);
/* Load the code objects of every translation unit of the library on the current device (one empty launch each on ``stream``):
 * what the first call of each kernel family would otherwise pay, 5-25 ms at a time, inside the reference's one-time
 * prepare_data (SubGNN/SubGNN.py:1024-1063).  Idempotent and cheap when they are loaded.  0 = ok. */
int sgnn_warm_up(void* stream);
/* last hip error string for SGNN_ERR_LAUNCH (static storage) */
const char* sgnn_last_error(void);

/* ---------------------------------------------------------------------------------------
 * a10  Structure-channel CSR gather: degree sequences of node sets.
 * Replaces gamma.get_degree_sequence (SubGNN/gamma.py:21-49) as called for every anchor patch
 * and every CC row at SubGNN/SubGNN.py:802-809.
 *   internal[i] = #neighbours of set_nodes[i] inside its set (self loop counts 2, networkx)
 *   external[i] = full_degree[id] - internal[i]; full_degree == NULL -> degree from the CSR
 * One entry per listed node (duplicates kept); if `sorted`, each set's entries are written
 * in ascending order (gamma.py:35,48).  out_external may be NULL.
 * self_loops (nullable): uint8[max_id + 1], number of self-loop entries in each node's CSR row;
 * when given, the kernel does not have to test every streamed neighbour against the row's owner.
 * max_set_size: upper bound on set length known to the caller (<= 64 selects the wavefront-per-set kernel; a set
 * that breaks the promise gets INT32_MIN in all its outputs, never stale memory).
 * set_order (nullable): int32[n_sets], a permutation: the order in which sets are handed to the
 * hardware dispatcher (results are unaffected); heaviest-first shortens the tail of the launch.
 * ------------------------------------------------------------------------------------- */
int sgnn_degree_sequence(const int64_t* rowptr, const int32_t* col, int64_t nnz,
                         const int32_t* full_degree, const uint8_t* self_loops,
                         const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                         int64_t max_set_size, int sorted,
                         int32_t* out_internal, int32_t* out_external, const int32_t* set_order, void* stream);
/* Same, for callers that also hold the CSR with every row's neighbour ids in ascending order
 * (col_sorted, same rowptr; a simple graph: no id twice in a row).  Lists of >= 512 entries are then
 * not streamed at all: every member of the set binary-searches its id in the list (log2(deg)
 * dependent loads for the whole set instead of deg/64 wave loads and table probes) -- on scale-free
 * graphs the hub lists carry most of the bytes.  Results are identical. */
int sgnn_degree_sequence_sorted_rows(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted,
                                     int64_t nnz, const int32_t* full_degree, const uint8_t* self_loops,
                                     const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                     int64_t max_set_size, int sorted, int32_t* out_internal,
                                     int32_t* out_external, const int32_t* set_order, void* stream);
/* Same, with membership BITMAPS for the long lists (built once per graph by the caller): hub_index[v] >= 0 numbers the
 * lists that have one, -1 = no bitmap for v; hub_bits holds one row of hub_words 32-bit words per NODE ID x (rows 0 ..
 * max id), bit hub_index[v] of row x = "x is in v's neighbour list" (laid out by node: one member's lookups against all
 * the hubs of its set share a cache line).  node_info (may be NULL; 16-byte aligned): one record of four int32 per node id
 * -- {row start, degree, hub number (0xffffff = none) | self-loop entries << 24, full degree} -- read INSTEAD of one line
 * each out of rowptr, hub_index, self_loops and full_degree (info_degree != 0: external = the record's full degree - internal,
 * else degree + self loops - internal).  A list of >= sgnn_degree_sequence_search_threshold() entries that has a bitmap is neither streamed
 * nor searched: every member of the set reads its one bit (gamma.get_degree_sequence, gamma.py:21-49: the membership test
 * `w in subgraph` for a hub's neighbours, asked from the set's side).  Such lists WITHOUT a bitmap are searched when
 * col_sorted is given (may be NULL), streamed otherwise.  Results are identical. */
int sgnn_degree_sequence_hub_bitmaps(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted,
                                     int64_t nnz, const int32_t* full_degree, const uint8_t* self_loops,
                                     const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words,
                                     const int32_t* node_info, int info_degree,
                                     const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                     int64_t max_set_size, int sorted, int32_t* out_internal,
                                     int32_t* out_external, const int32_t* set_order, void* stream);
int64_t sgnn_degree_sequence_search_threshold(void);
/* Sets of more than 2048 entries (components of subgraphs with thousands of nodes): the calls above leave them alone;
 * this one, issued after either on the same stream, writes their degrees UNSORTED (same counting rules; the membership
 * table lives in the workspace, sgnn_degree_sequence_huge_workspace_bytes(set_ptr[n_sets])); ordering such a set's slice
 * is the caller's (any segment sort). */
int64_t sgnn_degree_sequence_huge_workspace_bytes(int64_t total_entries);
int sgnn_degree_sequence_huge(const int64_t* rowptr, const int32_t* col, int64_t nnz, const int32_t* full_degree,
                              const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                              int64_t total_entries, int32_t* out_internal, int32_t* out_external,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a7  Connected components of induced subgraphs.
 * Replaces nx.connected_components(nx.subgraph(G, ids)) at SubGNN/SubGNN.py:589-592.
 * out_label[i] = smallest position (within its subgraph) of a node in the same component as
 * position i; duplicates of a node share a label.  Needs col_sorted.
 * ------------------------------------------------------------------------------------- */
int sgnn_cc_labels(const int64_t* rowptr, const int32_t* col_sorted, int64_t nnz,
                   const int64_t* sub_ptr, const int32_t* sub_nodes, int64_t n_subgraphs,
                   int64_t max_sub_len /* longest subgraph, 0 = unknown; subgraphs > 2048 nodes get -1: sgnn_cc_labels_huge */,
                   int32_t* out_label, void* stream);
/* Canonical order inside every set: ids ascending, equal ids in their original relative order.
 * The neighbourhood-anchor draw ranks "the ascending members" of a component / border set where the
 * reference walks a python set (SubGNN/anchor_patch_samplers.py:60-75, sample_neighborhood_anchor_patch);
 * this is the order both sides agree on.  out_pos (nullable): flat index the id came from, for
 * payloads that travel with the ids (hop labels).  max_set_size <= 1024, else SGNN_ERR_SET_TOO_LARGE
 * (the caller sorts (set, id) keys device-wide instead).  out_nodes must not alias set_nodes. */
int sgnn_sort_sets(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_size,
                   int32_t* out_nodes, int32_t* out_pos, void* stream);
/* labels -> the padded component tensor of SubGNN.initialize_cc_ids (SubGNN/SubGNN.py:575-607) in
 * canonical order: components by the position of their first node, nodes in subgraph order,
 * duplicates dropped, PAD = 0.  Two steps: _stats gives, per subgraph, the number of components and
 * the longest one (the caller takes the maxima C and L and zero-fills out (n_subgraphs, C, L) int64);
 * sgnn_cc_compact writes the ids.  max_sub_len: longest subgraph (0 = unknown); subgraphs of more than 2048 nodes are
 * skipped here and served by sgnn_cc_compact_huge below. */
int sgnn_cc_compact_stats(const int64_t* sub_ptr, const int32_t* sub_nodes, const int32_t* labels,
                          int64_t n_subgraphs, int64_t max_sub_len, int32_t* out_n_components,
                          int32_t* out_longest, void* stream);
int sgnn_cc_compact(const int64_t* sub_ptr, const int32_t* sub_nodes, const int32_t* labels,
                    int64_t n_subgraphs, int64_t max_sub_len, int64_t C, int64_t L, int64_t* out, void* stream);
/* The same three steps for subgraphs of MORE than 2048 nodes (the reference pads to any size, SubGNN/SubGNN.py:575-607):
 * the calls above leave such subgraphs alone (labels -1, no statistics, no rows) and these fill them in -- call them
 * after their counterpart on the same stream.  State lives in the caller's workspace
 * (sgnn_cc_huge_workspace_bytes(total_nodes), total_nodes = sub_ptr[n_subgraphs]; any content): id -> first position
 * table, union-find parents, ranks, counters, each subgraph at its own offset.  sgnn_cc_compact_huge: write == 0 gives
 * the statistics (out_n_components / out_longest), write != 0 the rows of out (n_subgraphs, C, L). */
int64_t sgnn_cc_huge_workspace_bytes(int64_t total_nodes);
int sgnn_cc_labels_huge(const int64_t* rowptr, const int32_t* col, int64_t nnz, const int64_t* sub_ptr,
                        const int32_t* sub_nodes, int64_t n_subgraphs, int64_t total_nodes, int32_t* out_label,
                        void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_cc_compact_huge(const int64_t* sub_ptr, const int32_t* sub_nodes, const int32_t* labels,
                         int64_t n_subgraphs, int64_t total_nodes, int write, int64_t C, int64_t L,
                         int32_t* out_n_components, int32_t* out_longest, int64_t* out, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a7b  Structural properties of induced subgraphs: what the DENSITY, CUT RATIO, CORENESS and COMPONENT labels of the
 * synthetic benchmarks are made of (reference prepare_dataset/prepare_dataset.py:519-550: nx.density, nx.edge_boundary,
 * nx.core_number, nx.number_connected_components of G.subgraph(nodes)), for all sets in one call.  Integer only.
 * A member is an entry v with 1 <= v <= max_id and a non-empty row; other entries (PAD included) are dropped, as
 * G.subgraph drops ids that are not nodes; a repeated member counts once.
 * out_counts int64 (n_sets, 6): {members, edges among them (no self loops, an undirected edge once, an id repeated inside
 * a row once), members with a self loop, boundary edges = distinct (member, non-member neighbour) pairs, connected
 * components, sum of the members' core numbers (self loops ignored)}.
 * out_core (nullable) int32, aligned with sub_nodes: the member's core number (repeats carry the same value), -1 for a
 * dropped entry.
 * rows_simple != 0: no row of col_sorted holds an id twice (the wave form then takes degree - self loop for a member's
 * distinct neighbours instead of reading the row).  max_len: longest set, 0 = unknown.  Sets of at most 64 entries take one
 * wavefront, sets of at most 2048 one workgroup with its tables in LDS; larger ones need max_len > 2048, total_nodes =
 * sub_ptr[n_sets] and a workspace of sgnn_subgraph_properties_workspace_bytes(total_nodes) bytes (any content), else
 * SGNN_ERR_BAD_ARG.  A set longer than max_len (or than 2048 with max_len unknown) gets -1 everywhere. */
int64_t sgnn_subgraph_properties_workspace_bytes(int64_t total_nodes);
int sgnn_subgraph_properties(const int64_t* rowptr, const int32_t* col_sorted, int64_t nnz, int64_t max_id, int rows_simple,
                             const int64_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sets, int64_t max_len,
                             int64_t total_nodes, int64_t* out_counts, int32_t* out_core, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a8  k-hop border of a component, and the hop level of each border node.
 * Replaces subgraph_utils.get_component_border_neighborhood_set (SubGNN/subgraph_utils.py:
 * 146-176) / SubGNN.initialize_border_sets (SubGNN/SubGNN.py:673-700).
 * Two-pass protocol: call with out_nodes == NULL to get out_count[s]; prefix-sum on the host
 * into out_ptr; call again with out_ptr/out_nodes (and optionally out_hop) to fill.  Entries
 * of a set come in discovery order (not sorted).
 * ego_dict_mode != 0 reproduces the `ego_graphs.txt` path (su:168-174): 1 hop only and every
 * border id is (true id - 1), differenced against the 1-based component (id 0 can appear).
 * bitmap_in_lds != 0 keeps the visited bitmap in the CU's LDS (allowed iff
 * sgnn_khop_border_bitmap_fits_lds(max_id)); the results are the same either way.
 * workspace: sgnn_khop_border_workspace_bytes(max_id, n_sets, bitmap_in_lds) bytes: per-workgroup
 * BFS queues and, for the global variant, the visited bitmaps, which must be ZERO on entry (they
 * are left zeroed, so one buffer can be reused across calls); the LDS variant needs no
 * initialisation.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_khop_border_workspace_bytes(int64_t max_id, int64_t n_sets, int bitmap_in_lds);
int sgnn_khop_border_bitmap_fits_lds(int64_t max_id);
int sgnn_khop_border(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                     const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                     int k, int ego_dict_mode,
                     int64_t* out_count, const int64_t* out_ptr, int32_t* out_nodes, uint8_t* out_hop,
                     void* workspace, int64_t workspace_bytes, int bitmap_in_lds, void* stream);
/* one-pass materialisation: slice s of `arena` (starting at arena_off[s], guaranteed by the caller to
 * hold the border: for k = 1, sum of the members' degrees always does) is used as the BFS queue, so
 * the border is written by the BFS itself; out_count[s] entries are valid, in discovery order. */
int sgnn_khop_border_arena(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                           const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int k,
                           const int64_t* arena_off, int32_t* arena, int64_t* out_count,
                           void* workspace, int64_t workspace_bytes, int bitmap_in_lds, void* stream);
/* a8 + a4 fused: k-hop border BFS and, without materialising the border, the neighbourhood-border
 * anchor draw of anchor_patch_samplers.sample_neighborhood_anchor_patch(sample_inside=False)
 * (anchor_patch_samplers.py:184-194) over it, under the neighbourhood-anchor law stated at
 * sgnn_sample_anchors_padded.  For set s and slot i (tape item (item_base + s)*n_slots+i; item_base = the
 * number of the first set when the sets are rows of a larger, sharded matrix): out_anchor = the k-th
 * smallest border id (a rank query on the visited bitmap -- no sort, no per-node hashing), out_hop =
 * its hop level (the N-border similarity, = the APSP row-min of SubGNN.py:772 on that column),
 * out_allneg = the item's "every variate negative" draw -- the caller applies the PAD rule of
 * aps:190 (PAD wins when it is set AND the padded row is longer than this border, i.e.
 * out_count[s] < max count).  An empty border yields anchor 0.
 * col_sorted (nullable): the rows in ascending order.  k = 1 takes a specialised kernel (bits ORed without
 * return value, a 16-lane group per slot); with col_sorted it also serves id ranges beyond the LDS bitmap
 * (~1.2 M ids) by processing the range in slices -- without it such graphs keep the bitmap in `workspace`.
 * bitmap_in_lds: 0 = bitmap in workspace, 1 = in LDS, > 1 = in LDS using at most this many bytes (smaller
 * slices; a test hook that needs no global state).  workspace: sgnn_khop_border_sample_workspace_bytes. */
int64_t sgnn_khop_border_sample_workspace_bytes(int64_t max_id, int64_t n_sets, int k, int rows_sorted, int bitmap_in_lds);
int sgnn_khop_border_sample(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz, int64_t max_id,
                            const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int k,
                            int64_t n_slots, uint64_t seed, uint64_t stream_id, int64_t item_base,
                            int64_t* out_anchor, uint8_t* out_hop, uint8_t* out_allneg, int64_t* out_count,
                            const int32_t* set_order /* nullable: dispatch order of the sets, a permutation */,
                            void* workspace, int64_t workspace_bytes, int bitmap_in_lds, void* stream);
/* The PAD rule of anchor_patch_samplers.py:189-191 on the drawn anchors, in place: slot := PAD where out_allneg is set and the
 * set's border is smaller than the padded matrix's width (width: device scalar, = max out_count, MAX-reduced over ranks when
 * the sets are one shard); sims (n_sets, n_slots) float32 := hop level, 0 on PAD. */
int sgnn_khop_sample_finish(int64_t* anchor, const uint8_t* hop, const uint8_t* allneg, const int64_t* counts,
                            const int64_t* width, int64_t n_sets, int64_t n_slots, float* sims, void* stream);
/* The one-hop border of every set WRITTEN in ascending id order by the one-hop kernel's own rank pass (no sort): for a caller
 * whose sets stay the same from call to call, which then draws with sgnn_sample_border_anchors instead of rebuilding the border
 * inside sgnn_khop_border_sample.  Two calls: out_ids == NULL writes out_count[s] only; with out_ptr (the caller's exclusive
 * prefix sum of the counts, n_sets + 1 entries) and out_ids, set s's border goes to out_ids[out_ptr[s] .. out_ptr[s+1])
 * (out_count, if given, is written again).  col_sorted, bitmap_in_lds and workspace (16 bytes: the set counter) as for
 * sgnn_khop_border_sample with k = 1 -- but where that call would leave its specialised kernel (no LDS plan for the id range,
 * or slices needed and col_sorted == NULL) this one returns SGNN_ERR_SET_TOO_LARGE and writes nothing. */
int sgnn_khop1_border_sorted(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz, int64_t max_id,
                             const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                             int64_t* out_count, const int64_t* out_ptr /* nullable */, int32_t* out_ids /* nullable */,
                             void* workspace, int64_t workspace_bytes, int bitmap_in_lds, void* stream);

/* Padded id rows (n_rows, row_len) int64 -> ragged sets: PAD (0) entries stripped -- or, with mask (uint8, same shape), the
 * entries whose mask is 0 -- order kept (how gamma.py:27, anchor_patch_samplers.py:131 and SubGNN.py:769 strip PAD).
 * sgnn_pack_rows_count writes the rows' kept counts; the caller's exclusive prefix sum of them is ptr (n_rows + 1);
 * sgnn_pack_rows_write writes the kept ids (as int32) behind ptr[row]. */
/* keep (n_rows, row_len) uint8: 1 where ids[r, i] != PAD and no earlier entry of the row holds the same id -- the node view of
 * a patch (unique nodes of a walk, first occurrence first: anchor_patch_samplers.py:131-138) as a mask for sgnn_pack_rows_*. */
int sgnn_first_occurrence_mask(const int64_t* ids, int64_t n_rows, int64_t row_len, uint8_t* keep, void* stream);
/* The flagged entries (flags uint8, aligned with set_nodes) of every ragged set, order kept -- a patch's in-border nodes
 * (subgraph_utils.py:126-144 via sgnn_patch_in_border).  counts != NULL: write the sets' flagged counts; counts == NULL: write
 * the flagged ids behind out_ptr[set] (the caller's exclusive prefix sum of the counts). */
int sgnn_filter_sets(const int64_t* set_ptr, const int32_t* set_nodes, const uint8_t* flags, int64_t n_sets, int64_t* counts,
                     const int64_t* out_ptr, int32_t* out_nodes, void* stream);
int sgnn_pack_rows_count(const int64_t* ids, const uint8_t* mask, int64_t n_rows, int64_t row_len, int64_t* counts,
                         void* stream);
int sgnn_pack_rows_write(const int64_t* ids, const uint8_t* mask, int64_t n_rows, int64_t row_len, const int64_t* ptr,
                         int32_t* nodes, void* stream);
/* The same packings in ONE launch for up to sgnn_pack_fused_max_rows() rows / sets (the few hundred structure patches of a pass:
 * anchor_patch_samplers.py:131-138 node views, subgraph_utils.py:126-144 in-border sets, gamma.py:27 PAD stripping): counts,
 * prefix sum, packed write and the zeroed tail of the arena by one workgroup.  mode 0: keep non-PAD ids; 1: keep where
 * mask != 0; 2: keep non-PAD ids that no earlier entry of the row repeats (first occurrence).  ptr: n_rows + 1 entries
 * (all written); nodes: an arena of n_rows * row_len + 1 entries (all written).  sgnn_filter_sets_fused: out_nodes is an arena
 * of arena_entries entries (>= the flagged total), all written. */
int64_t sgnn_pack_fused_max_rows(void);
int64_t sgnn_pack_fused_max_entries(void);   /* n_rows * row_len (the sets' arena for the filter) may not exceed this: entries are staged in LDS */
int sgnn_pack_rows_fused(const int64_t* ids, const uint8_t* mask, int mode, int64_t n_rows, int64_t row_len, int64_t* ptr,
                         int32_t* nodes, void* stream);
int sgnn_filter_sets_fused(const int64_t* set_ptr, const int32_t* set_nodes, const uint8_t* flags, int64_t n_sets,
                           int64_t arena_entries, int64_t* out_ptr, int32_t* out_nodes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a4  Neighbourhood anchor sampling from padded id matrices.
 * Replaces anchor_patch_samplers.sample_neighborhood_anchor_patch (anchor_patch_samplers.py:
 * 163-198).  The reference draws one N(0,1) variate per column, zeroes the PAD columns and takes
 * the argmax (aps:177-179,189-191); in law: each non-PAD entry equally likely, except that PAD wins
 * when all n real variates are negative (probability 2^-n) and the row has a PAD column.  The
 * tape's neighbourhood-anchor law states exactly that with two draws of item r*n_slots+i:
 *   draw 0: index (u32 * n) >> 32 into the row's non-PAD entries in ASCENDING id order;
 *   draw 1: "every variate negative" iff n <= 32 and the top n bits of u32 are zero.
 * ids: (n_rows, L) int64 in CANONICAL form -- non-PAD entries ascending, PADs (0) last;
 * out (n_rows, n_slots).  (subgnn_amd.ops canonicalises arbitrary rows before the call.)
 * ------------------------------------------------------------------------------------- */
int sgnn_sample_anchors_padded(const int64_t* ids, int64_t n_rows, int64_t L, int64_t n_slots,
                               uint64_t seed, uint64_t stream_id, int64_t* out, void* stream);
/* same law on ragged sets, each ascending; row_has_pad[r] (nullable = all 1) says whether the
 * padded row would hold a PAD.  item_base: number of the first set within the whole (possibly
 * sharded) matrix -- set r draws as tape item (item_base + r)*n_slots + slot, so a shard of the rows
 * reproduces the draws of the unsharded call. */
int sgnn_sample_anchors_ragged(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                               const uint8_t* row_has_pad, int64_t n_slots,
                               uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t* out, void* stream);
/* The neighbourhood-border draw on kept sorted borders (sgnn_khop1_border_sorted: ptr, ids, counts), one launch: the law of
 * sgnn_sample_anchors_ragged with row_has_pad[r] = counts[r] < width[0] (width: DEVICE scalar, the padded border matrix's width)
 * and out_sims (n_sets, n_slots) float32 = hop where the anchor is a node, 0 on PAD -- bit for bit what sgnn_khop_border_sample
 * followed by sgnn_khop_sample_finish write for k = hop = 1.  An empty border gives anchor 0, similarity 0. */
int sgnn_sample_border_anchors(const int64_t* ptr, const int32_t* ids, const int64_t* counts, int64_t n_sets,
                               const int64_t* width, int64_t n_slots, uint64_t seed, uint64_t stream_id, int64_t item_base,
                               int hop, int64_t* out_anchor, float* out_sims, void* stream);

/* ---------------------------------------------------------------------------------------
 * a5/a6  Uniform draws with replacement from a list (position anchors, structure picks).
 * Replaces np.random.choice(seq, n, replace=True) at anchor_patch_samplers.py:206,208,326.
 * list r draws as tape item item_base + r from seq[ptr[r] .. ptr[r+1]); out (n_items, n_draws) int64.
 * ------------------------------------------------------------------------------------- */
int sgnn_choice_ragged(const int64_t* ptr, const int32_t* seq, int64_t n_items, int64_t n_draws,
                       uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * a4-a6 keyed  The same draws for sets that are no rows of a split (prediction on subgraphs outside the dataset).
 * The reference ties every draw to the row's place in its split: the serial RNG is consumed row by row
 * (anchor_patch_samplers.py:177,189,206,208) and the PAD rule compares a row with the widest row of the same matrix
 * (anchor_patch_samplers.py:178,190).  Here the tape item comes from a caller-supplied 64-bit key per set and the PAD rule from
 * a caller-supplied flag per set, so a set's draw is a function of (seed, stream, key, flag, content) and of nothing else in the
 * list.
 *
 * sgnn_set_keys: out_keys[s] (uint64) = a key of the CONTENT of ragged set s, independent of the order of its entries:
 *     key = sgnn_mix64( (sum over the n entries v of sgnn_mix64(v)) + (n + 1) * 0x8CB92BA72F3D8DD7 )
 * in uint64 wrap-around arithmetic (v: the int32 id zero-extended; sgnn_mix64: the tape's splitmix64 finaliser).  The sum
 * commutes; a repeated entry changes both the sum and n; the empty set has key sgnn_mix64(0x8CB92BA72F3D8DD7).  One wavefront
 * per set.  Host twin: subgnn_amd.tape.set_key_np.
 *
 * sgnn_sample_anchors_ragged_keyed: the law of sgnn_sample_anchors_ragged; set r, slot i draws as tape item
 * keys[r]*n_slots + i (uint64 wrap-around); row_has_pad (uint8, required) as there.
 * sgnn_choice_ragged_keyed: the law of sgnn_choice_ragged; list r draws as tape item keys[r].
 * sgnn_sample_border_anchors_keyed: the law of sgnn_sample_border_anchors on ascending borders of ANY depth
 * (neigh_sample_border_size: SubGNN.py:673-700) with hops[e] (uint8, aligned with ids) the hop level of entry e: item
 * keys[r]*n_slots + i, row_has_pad[r] in place of counts[r] < width[0], out_sims = the drawn entry's hop, 0 on PAD.
 * With keys[r] = item_base + r (and, for the border form, row_has_pad = counts < width, hops = hop) each writes the bits of its
 * unkeyed twin.  An empty set gives anchor 0 (similarity 0).
 * ------------------------------------------------------------------------------------- */
int sgnn_set_keys(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, uint64_t* out_keys, void* stream);
int sgnn_sample_anchors_ragged_keyed(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                                     const uint8_t* row_has_pad, const uint64_t* keys, int64_t n_slots,
                                     uint64_t seed, uint64_t stream_id, int64_t* out, void* stream);
int sgnn_choice_ragged_keyed(const int64_t* ptr, const int32_t* seq, int64_t n_items, const uint64_t* keys, int64_t n_draws,
                             uint64_t seed, uint64_t stream_id, int64_t* out, void* stream);
int sgnn_sample_border_anchors_keyed(const int64_t* ptr, const int32_t* ids, const uint8_t* hops, int64_t n_sets,
                                     const uint8_t* row_has_pad, const uint64_t* keys, int64_t n_slots, uint64_t seed,
                                     uint64_t stream_id, int64_t* out_anchor, float* out_sims, void* stream);

/* ---------------------------------------------------------------------------------------
 * Occlusion sets (no reference counterpart): every leave-one-unit-out variant of every ragged set, for attribution by
 * occlusion on subgraphs outside the dataset.  The entries of every set are ascending and without repeats (sgnn_sort_sets).
 *   mode SGNN_OCC_NODE       every entry is a unit; the rank of a unit is its position
 *   mode SGNN_OCC_COMPONENT  every component is a unit: labels (int32, aligned with set_nodes, required) are those of
 *                            sgnn_cc_labels -- the smallest position in the set of an entry of the same component; units are
 *                            ranked by their smallest position (the order of sgnn_cc_compact).  An entry whose label is no
 *                            position before it that labels itself is a unit of its own (nothing is read out of bounds).
 * A unit whose removal leaves nothing produces no variant: a set of fewer than two units has none.  Every other unit u
 * produces the set without u's entries, order kept (so ascending: no sort follows).
 *
 * sgnn_occlusion_count: out_units[s], out_variants[s] (int64) and out_len (int64, one slot per ENTRY of the input, zeroed
 * by the caller): slot set_ptr[s] + u = the length of the variant of unit u of set s, 0 where there is none.  The caller's
 * exclusive prefix sums are var_ptr (of out_variants, n_sets + 1) and len_scan (of out_len, one per slot): their last
 * values -- the number of variants and of their entries -- size the outputs of
 * sgnn_occlusion_write: the variant of unit u of set s is variant v = var_ptr[s] + u: out_ptr[v] = len_scan[set_ptr[s] + u]
 * (and out_ptr[n_variants] behind the last), its entries in out_nodes from there, out_parent[v] = s, out_unit[v] = u and
 *     out_keys[v] = sgnn_mix64( sum_parent - (sum over the removed entries r of sgnn_mix64(r)) + (n_variant + 1) * 0x8CB92BA72F3D8DD7 )
 * in uint64 wrap-around arithmetic: the bits sgnn_set_keys gives for the variant, from one sum over the parent (the variant
 * is not read again).
 * A set is read once; all its variants are written from a copy in LDS (up to sgnn_occlusion_lds_max() entries; up to 64 a
 * wavefront per set), one wavefront writing a variant front to back.  Longer sets are streamed from global memory, in
 * component mode with their unit tables in the caller's workspace (sgnn_occlusion_workspace_bytes(total_entries) bytes, 16 per
 * entry of the input; may be NULL when max_set_len says no set is that long).  max_set_len: the longest set, 0 = unknown.
 * n_sets < 2^31.
 * ------------------------------------------------------------------------------------- */
#define SGNN_OCC_NODE 0
#define SGNN_OCC_COMPONENT 1
int64_t sgnn_occlusion_lds_max(void);
int64_t sgnn_occlusion_workspace_bytes(int64_t total_entries);
int sgnn_occlusion_count(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len, int mode,
                         const int32_t* labels, int64_t* out_units, int64_t* out_variants, int64_t* out_len,
                         int64_t total_entries, void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_occlusion_write(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len, int mode,
                         const int32_t* labels, const int64_t* var_ptr, const int64_t* len_scan, int64_t n_variants,
                         int64_t* out_ptr, int32_t* out_nodes, int32_t* out_parent, int32_t* out_unit, uint64_t* out_keys,
                         int64_t total_entries, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Insertion sets (no reference counterpart): every add-one-candidate variant of every ragged set, for scoring the nodes a
 * subgraph outside the dataset could gain.  A set is ascending and without repeats (sgnn_sort_sets); it may be empty.  A
 * candidate row is the same.  The candidates are cand_ptr (int64) / cand_ids (int32):
 *   shared 0   one candidate row per set (n_sets + 1 pointers)
 *   shared 1   ONE row (two pointers) that every set takes (a pool is not replicated per set)
 * The variants of set s of n entries are, in the order of its candidate row, one per candidate v that is no member of s: the
 * ascending set s U {v} of n + 1 entries (so no sort follows).  A candidate that is a member is skipped, not an error; the
 * variants of an empty set are the singletons.
 *
 * sgnn_insertion_count: out_variants[s] (int64) = the number of candidates of set s that are no members.  The caller's
 * exclusive prefix sums are var_ptr (of out_variants) and entry_ptr (of out_variants[s] * (n_s + 1)), n_sets + 1 each: their
 * last values -- the number of variants and of their entries -- size the outputs of
 * sgnn_insertion_write: the k-th variant of set s is variant v = var_ptr[s] + k: out_ptr[v] = entry_ptr[s] + k (n_s + 1) (and
 * out_ptr[n_variants] behind the last), its entries in out_nodes from there, out_parent[v] = s, out_cand[v] = the inserted id
 * (int32 both) and
 *     out_keys[v] = sgnn_mix64( sum_parent + sgnn_mix64(v) + (n_s + 2) * 0x8CB92BA72F3D8DD7 )
 * in uint64 wrap-around arithmetic: the bits sgnn_set_keys gives for the variant, from one sum over the parent (the variant
 * is not read again).
 * One workgroup per set: the set is read once (into LDS up to 1024 entries; up to 64 a wavefront per set; longer ones are
 * read from global memory), the candidate row in chunks of one candidate per thread, each placed by a binary search in the
 * set.  max_set_len: the longest set, 0 = unknown.  n_sets and n_variants < 2^31.  SGNN_ERR_BAD_ARG, with nothing written,
 * for negative sizes, sizes beyond that, shared outside {0, 1}, a NULL input with sets to read or a NULL output with variants
 * to write.
 * ------------------------------------------------------------------------------------- */
int sgnn_insertion_count(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len,
                         const int64_t* cand_ptr, const int32_t* cand_ids, int shared, int64_t* out_variants, void* stream);
int sgnn_insertion_write(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, int64_t max_set_len,
                         const int64_t* cand_ptr, const int32_t* cand_ids, int shared, const int64_t* var_ptr,
                         const int64_t* entry_ptr, int64_t n_variants, int64_t* out_ptr, int32_t* out_nodes,
                         int32_t* out_parent, int32_t* out_cand, uint64_t* out_keys, void* stream);

/* ---------------------------------------------------------------------------------------
 * Seeded walk sets: many connected candidate subgraphs around seed nodes, for finding further subgraphs of a class.  The
 * reference has no counterpart; the nearest is its random-walk patch sampling (anchor_patch_samplers.py:20-113), whose walks
 * are kept as sequences.  Here the SET of visited nodes is the result, ascending and with its content key, as the other set
 * entries take it.
 *
 * The graph is rowptr (int64, max_id + 2) / col (int32): node ids 1 .. max_id, row 0 (PAD) empty, rows ascending, every edge
 * in both rows.  seeds: int32[n_seeds].  sizes: int32[per_seed], the target size of candidate c of every seed; a value outside
 * 1 .. width counts as clamped to it.  Item number q is item_ids[i] (int64[n_items]) if item_ids is given, else
 * item_base + i; its seed is s = seeds[q / per_seed], its size sizes[q % per_seed].  Its draws come from
 *     h1 = sgnn_tape_h1(sgnn_tape_h0(seed, stream), q)
 * -- the item NUMBER, not the output row i: a chunk (item_base) or a list of items gives the bits of those rows of the whole
 * call, so a caller may keep item numbers and regenerate their sets later.
 *
 * The walk: cur = s, set = {s}, t = 0.  A seed outside 1 .. max_id (or, with item_ids, q < 0 or q / per_seed >= n_seeds) gives
 * the empty set with 0 steps; a seed without an edge gives {s} with 0 steps.  Otherwise, while |set| < size and t < max_steps:
 *     r = (uint32)(sgnn_tape_draw(h1, 2t) >> 32)
 *     (uint64) r < restart_thr:  cur = s
 *     else:  d = rowptr[cur + 1] - rowptr[cur],  cur = col[rowptr[cur] + sgnn_choice_index(h1, 2t + 1, d)],  and cur joins
 *            the set if it is no member (a row without entries, which only a one-way CSR has here, sends the walk to s)
 *     t += 1
 * cur is always a member, so every node that joins is adjacent to one: the set induces a connected subgraph that holds s.
 * restart_thr is the restart probability in units of 2^-32, 0 .. 2^32 (the caller forms min(2^32, floor(p * 2^32)): no float
 * arithmetic runs on the device).
 *
 * Row i of the outputs: out_nodes[i * width ..] the set ascending, then zeros up to width; out_len[i], out_steps[i] (the final
 * t) int32; out_keys[i] = sgnn_set_key_finish(sum of sgnn_mix64(v), len): the bits sgnn_set_keys gives for the set.
 * One wavefront per item; the set is held in four registers of every lane, width <= sgnn_seeded_walk_max_size() = 256.
 * SGNN_ERR_BAD_ARG, with nothing written, for negative max_id, n_seeds, n_items, item_base or max_steps, width < 1 or above
 * the maximum, per_seed < 1, restart_thr > 2^32, n_items or max_steps > 2^31 - 1, item_base + n_items > n_seeds * per_seed
 * without item_ids, and a NULL pointer with items to write (seeds may be NULL for n_seeds = 0).  n_items = 0 writes nothing.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_seeded_walk_max_size(void);
int sgnn_seeded_walk_sets(const int64_t* rowptr, const int32_t* col, int64_t max_id, const int32_t* seeds, int64_t n_seeds,
                          const int32_t* sizes, int64_t per_seed, int64_t width, uint64_t restart_thr, int64_t max_steps,
                          uint64_t seed, uint64_t stream, int64_t item_base, const int64_t* item_ids, int64_t n_items,
                          int32_t* out_nodes, int32_t* out_len, int32_t* out_steps, uint64_t* out_keys, void* stream_handle);

/* ---------------------------------------------------------------------------------------
 * Node overlap of ragged node sets.  The reference has no counterpart: it compares subgraphs through the model only.
 *
 * A SET is an ascending int32 array without repeats, ids >= 0; it may be empty.  A BANK is n_rows sets (bank_ptr: int64,
 * n_rows + 1; only the sizes are read) with its POSTINGS: post_rows[post_ptr[v] .. post_ptr[v + 1]) (post_ptr int64,
 * max_id + 2 entries; post_rows int32) are, ascending, the bank rows that hold node v.  A query id above max_id is held by no
 * row.  The number of postings a set walks is P = sum over its members v <= max_id of post_ptr[v + 1] - post_ptr[v]; the
 * caller passes it per set.  It decides where the set's counting table lives: P <= sgnn_overlap_lds_max() (2048) in LDS,
 * beyond it in the workspace, in the region at the set's offset (q_ws_off[s], in postings: the exclusive prefix sums of the P
 * of the sets beyond the LDS tier; ws_entries = their sum <= 2^28, workspace of sgnn_overlap_workspace_bytes(ws_entries)
 * bytes, < 0 for a count the calls refuse).  A set beyond the LDS tier whose region the workspace does not hold gets fillers.
 * Results never depend on the home.
 *
 * sgnn_overlap_topk: for every query q the k <= sgnn_overlap_max_k() (64) best bank rows b among those with i = |q n b| >= 1,
 * best first.  The measure is a fraction num / den:
 *     SGNN_OVL_JACCARD      i / (|q| + |b| - i)
 *     SGNN_OVL_CONTAINMENT  i / |q|
 *     SGNN_OVL_COVERAGE     i / |b|
 *     SGNN_OVL_COUNT        i / 1
 * The order is exact: the larger fraction first, compared by n1 * d2 against n2 * d1 in 64 bits (every factor < 2^31), never
 * through a quotient; equal fractions by the smaller row.  It is strict and total.  exclude (nullable): per query a bank row to
 * skip, or -1.  out_rows (Q, k) int64, fillers -1; out_inter (Q, k) int32, the i of those rows, fillers 0; out_touched (Q)
 * int32: the number of bank rows with i >= 1, the excluded one included.  One workgroup per query.
 *
 * sgnn_overlap_diverse: greedy selection among n_sets sets given in rank order (row r is rank r) with their OWN postings (the
 * bank is the sets themselves), the threshold tau = tau_num / tau_den (0 <= tau_num <= tau_den <= 2^20) and top >= 1:
 *     accepted = []; by = [-1] * N
 *     for r in 0 .. N-1:
 *         if by[r] >= 0: continue
 *         accepted.append(r)
 *         if len(accepted) == top: break
 *         for every c > r with by[c] < 0 and i(r,c) * tau_den > tau_num * (|r| + |c| - i(r,c)):
 *             by[c] = r
 * (a pair with an empty union shares nothing and is never too similar).  out_accepted (top) int64, fillers -1; out_n (1)
 * int32 = len(accepted); out_suppressed_by (N) int32 = by.  ONE launch of one workgroup, which reads nothing back; its
 * workspace holds one region: ws_entries >= the largest P beyond the LDS tier (0: none is).
 *
 * SGNN_ERR_BAD_ARG before any launch, with nothing written, for negative sizes, sizes or max_id above 2^31 - 1, k, measure,
 * tau or top outside their ranges, a workspace smaller than its query says, and a NULL pointer that the call would read or
 * write (q_ws_off and the workspace may be NULL with ws_entries = 0).  n_queries = 0 writes nothing.
 * ------------------------------------------------------------------------------------- */
#define SGNN_OVL_JACCARD     0
#define SGNN_OVL_CONTAINMENT 1
#define SGNN_OVL_COVERAGE    2
#define SGNN_OVL_COUNT       3
int64_t sgnn_overlap_max_k(void);
int64_t sgnn_overlap_lds_max(void);
int64_t sgnn_overlap_workspace_bytes(int64_t entries);
int sgnn_overlap_topk(const int64_t* q_ptr, const int32_t* q_nodes, int64_t n_queries, const int64_t* q_postings,
                      const int64_t* q_ws_off, const int64_t* bank_ptr, int64_t n_rows, const int64_t* post_ptr,
                      const int32_t* post_rows, int64_t max_id, const int64_t* exclude, int64_t k, int measure,
                      void* workspace, int64_t ws_entries, int64_t workspace_bytes, int64_t* out_rows, int32_t* out_inter,
                      int32_t* out_touched, void* stream);
int sgnn_overlap_diverse(const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets, const int64_t* set_postings,
                         const int64_t* post_ptr, const int32_t* post_rows, int64_t max_id, int64_t tau_num, int64_t tau_den,
                         int64_t top, void* workspace, int64_t ws_entries, int64_t workspace_bytes, int64_t* out_accepted,
                         int32_t* out_n, int32_t* out_suppressed_by, void* stream);

/* ---------------------------------------------------------------------------------------
 * a1-a3  Triangular random walks.
 * Replaces anchor_patch_samplers.triangular_random_walk / perform_random_walks /
 * sample_structure_anchor_patches (anchor_patch_samplers.py:20-158, 210-243).
 *   mode 0  'graph' : start = uniform over node_order (aps:70 with the whole graph)
 *   mode 1  'inside': walk inside the induced subgraph of patch p = item / walks_per_patch;
 *                     start uniform over the patch's node view  patch_ptr/patch_nodes (unique)
 *   mode 2  'border': start uniform over in_border nodes (inb_ptr/inb_nodes); neighbours
 *                     restricted to in_border U (V \ patch) (aps:141-143)
 * out: (n_items, walk_len) int64, PAD filled.  One tape item per walk (item = item_base + walk index: a rank that runs a
 * share of a launch's walks -- with the patches of that share only, for modes 1 and 2 -- draws what the whole launch would).
 * sgnn_triangular_walks_both: the internal AND the border walks over the same patches (aps:118-158, which the reference calls
 * twice: inside = True / False) in ONE launch, on every graph: out (2, n_items, walk_len), [0] = internal walks (tape stream
 * stream_id_int), [1] = border walks (stream_id_bor) -- the walks the two calls of sgnn_triangular_walks (modes 1, 2) produce.
 *
 * Three kernels give the same walks; they differ in how "is candidate w adjacent to the previous node?" is answered:
 *   bitmap     a workgroup of 1024 threads and a CU per walk; an LDS bitmap over node ids holds N(prev): one bit test.  Only
 *              where the bitmap fits (max_id, the largest id -- rowptr has max_id + 2 entries; 0 = unknown -- below ~1.1 M)
 *   list       a workgroup per walk, a few KB of LDS, several walks per CU, no limit on ids.  N(prev) staged in LDS as a hash
 *              when it has fewer than 512 entries; else bit hub_index[prev] of row w of the hub tables (hub_index / hub_bits /
 *              hub_words as for sgnn_degree_sequence_hub_bitmaps; both NULL: no tables); else a binary search in col_sorted
 *   wavefront  a wavefront per walk, binary search in col_sorted: the device-side reference of the other two
 * kernel: 0 = the workgroup kernels, as variant says; 1 = the wavefront kernel (it has no combined launch:
 * sgnn_triangular_walks_both returns SGNN_ERR_BAD_ARG); 2 = the bitmap kernel whatever the size of the launch, or
 * SGNN_ERR_SET_TOO_LARGE, before any launch, where max_id <= 0 or the bitmap does not fit (tests and measurements).
 * variant (kernel 0): 0 = the launch rule -- launches of up to 256 walks (a CU for every walk) on a graph whose bitmap fits go
 * to the bitmap kernel, which is faster there; all others to the list kernel with 512 threads; 1 ..
 * sgnn_triangular_walks_variants() - 1 = the list kernel always, at 256 / 512 / 1024 threads with a 256-chunk ballot cache,
 * 512 threads with 1024 chunks (same walks; for tests and measurements).
 * ------------------------------------------------------------------------------------- */
int sgnn_triangular_walks_variants(void);
/* 1 = variant 0 sends a launch of n_walks walks (internal + border counted together) to the bitmap kernel: the caller need
 * not have hub tables.  Tuned on the benchmark's hub-heavy graph. */
int sgnn_triangular_walks_rule(int64_t n_walks, int64_t max_id);
int sgnn_triangular_walks(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz,
                          const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words,
                          const int32_t* node_order, int64_t n_nodes,
                          const int64_t* patch_ptr, const int32_t* patch_nodes,
                          const int64_t* inb_ptr, const int32_t* inb_nodes,
                          int mode, int64_t n_items, int64_t walks_per_patch, int64_t walk_len, double beta,
                          uint64_t seed, uint64_t stream_id, int64_t item_base, int64_t max_id, int kernel, int variant,
                          int64_t* out, void* stream);
int sgnn_triangular_walks_both(const int64_t* rowptr, const int32_t* col, const int32_t* col_sorted, int64_t nnz,
                               const int32_t* hub_index, const uint32_t* hub_bits, int64_t hub_words,
                               const int64_t* patch_ptr, const int32_t* patch_nodes, const int64_t* inb_ptr,
                               const int32_t* inb_nodes, int64_t n_items, int64_t walks_per_patch, int64_t walk_len,
                               double beta, uint64_t seed, uint64_t stream_id_int, uint64_t stream_id_bor,
                               int64_t item_base, int64_t max_id, int kernel, int variant, int64_t* out, void* stream);

/* in-border nodes of a patch (subgraph_utils.get_border_nodes, subgraph_utils.py:126-144, with
 * its id-1 / node-order indexing quirk): out_flag[i] = 1 iff patch_nodes[i] is a border node.
 * node_order[i] = id at position i of G.nodes(); node_pos[id] = position (0-based). */
int sgnn_patch_in_border(const int64_t* rowptr, const int32_t* col, int64_t nnz,
                         const int32_t* node_order, const int32_t* node_pos, int64_t n_nodes,
                         const int64_t* patch_ptr, const int32_t* patch_nodes, int64_t n_patches,
                         uint8_t* out_flag, void* stream);
/* Patches of more than 2048 nodes (ego-graph patches around hubs): the call above marks their flags 255 and this one,
 * issued after it on the same stream, fills them in; the membership table lives in the workspace
 * (sgnn_patch_in_border_huge_workspace_bytes(total_nodes), total_nodes = patch_ptr[n_patches]). */
int64_t sgnn_patch_in_border_huge_workspace_bytes(int64_t total_nodes);
int sgnn_patch_in_border_huge(const int64_t* rowptr, const int32_t* col, int64_t nnz,
                              const int32_t* node_order, const int32_t* node_pos, int64_t n_nodes,
                              const int64_t* patch_ptr, const int32_t* patch_nodes, int64_t n_patches,
                              int64_t total_nodes, uint8_t* out_flag, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* ---------------------------------------------------------------------------------------
 * a9  Shortest-path similarities.
 * Replaces SubGNN.compute_shortest_path_similarities (SubGNN/SubGNN.py:752-781), dense-parity
 * form: out[r, :] = min over v in set r of apsp[v-1, :] (float64 in, float32 out), empty set
 * -> PAD.  apsp: (n, n_cols) row-major.
 * ------------------------------------------------------------------------------------- */
int sgnn_sp_similarity_dense(const double* apsp, int64_t n_cols,
                             const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                             float* out, void* stream);
/* sparse form for graphs where the N x N matrix cannot exist: hop distance from each of
 * n_sources source nodes to every node, by a level-synchronous bit-parallel multi-source BFS
 * (64 sources per machine word).  dist: (n_sources, max_id + 1) uint8, 255 = not reached within
 * max_hops (the reference's matrix holds 0 for unreachable pairs, precompute_graph_metrics.py:
 * 20-25; sgnn_min_hops_to_sets applies that convention).
 * workspace: sgnn_bfs_hops_workspace_bytes(max_id, n_sources, max_hops) bytes (any content).
 * The expansion is direction-optimising: a level pulls (every incomplete node ORs its neighbours'
 * frontier words) instead of pushing once the frontier's edge volume exceeds 1/alpha of all edges.
 * pull_alpha: that alpha (negative = the default, 32; 0 = always push); results do not depend on it. */
int64_t sgnn_bfs_hops_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops);
int sgnn_bfs_hops(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                  const int32_t* sources, int64_t n_sources, int max_hops, int node_major, int pull_alpha,
                  uint8_t* dist, void* workspace, int64_t workspace_bytes, void* stream);
/* out[r, a] = min over v in set r of (dist[a, v] == 255 ? 0 : dist[a, v])  (float32; empty set -> 0) */
/* node_major != 0: dist is laid out (max_id + 1, n_sources) instead -- the sources of a node are
 * contiguous, which coalesces both the BFS writes and the per-(set, source) min below */
int sgnn_min_hops_to_sets(const uint8_t* dist, int64_t n_sources, int64_t max_id, int node_major,
                          const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                          float* out, void* stream);
/* both steps in one: out[r, s] = min over the members of set r of the hop distance from source s
 * (0 when some member is unreachable from s: the reference's matrix holds 0 there and its row-min
 * runs over it) -- compute_shortest_path_similarities
 * (SubGNN/SubGNN.py:752-781) restricted to the anchor columns, without the (sources x nodes) hop
 * table: after every BFS level each set ORs its members' new frontier words and records the level for
 * the sources it sees for the first time.  out: (n_sets, n_sources) float32.
 * All max_hops levels are enqueued without a host synchronisation (levels behind the last productive one exit at
 * once).  out_status (nullable, int32[4], device): [0] = the last level that found anything, [1] = 1 if level
 * max_hops itself still did -- the caller enqueued too few levels and the result may be incomplete, [2] = the first
 * level that pulled (0: none), [3] = 0.  A caller that repeats the same search (the same graph and anchors every pass)
 * can read [0] once and pass max_hops = [0] + a margin afterwards, checking [1] at its next synchronisation point.
 * push_levels: the levels that may still push -- each costs a commit launch besides its expand launch; beyond them a
 * level pulls whatever its frontier (one launch: a pull level writes the next version of the seen rows itself).
 * < 0: all of them.  Results do not depend on it; a repeated search passes [2] + a margin. */
int64_t sgnn_bfs_min_hops_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops, int64_t n_sets);
int sgnn_bfs_min_hops_to_sets(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                              const int32_t* sources, int64_t n_sources, int max_hops, int pull_alpha, int push_levels,
                              const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                              float* out, int32_t* out_status, void* workspace, int64_t workspace_bytes, void* stream);
/* labels[v] = the smallest node id of v's connected component, for every id 0..max_id (int32; ids without edges, the pad
 * id 0 among them, label themselves).  The CSR is taken as undirected.  Synchronises the stream (one word is read back per
 * round): meant to run once per graph, outside any capture. */
int64_t sgnn_graph_component_labels_workspace_bytes(int64_t max_id);
int sgnn_graph_component_labels(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                                int32_t* labels, void* workspace, int64_t workspace_bytes, void* stream);
/* sgnn_bfs_min_hops_to_sets that stops once every set has its hops.  On a symmetric CSR a source reaches a member iff both
 * carry the same component label (labels: sgnn_graph_component_labels), so the pairs that will ever hold a level are known
 * up front; when all of them are recorded the search is closed and every later launch returns at once.
 * Values: those of sgnn_bfs_min_hops_to_sets bit for bit whenever out_status[1] == 0.  out_status: [0] = the closing level,
 * else the last level that found anything; [1] = 1 only if the enqueued levels ran out before the search closed and before
 * the frontier died; [2], [3] as above. */
int64_t sgnn_bfs_min_hops_closing_workspace_bytes(int64_t max_id, int64_t n_sources, int max_hops, int64_t n_sets);
int sgnn_bfs_min_hops_to_sets_closing(const int64_t* rowptr, const int32_t* col, int64_t nnz, int64_t max_id,
                                      const int32_t* sources, int64_t n_sources, int max_hops, int pull_alpha, int push_levels,
                                      const int32_t* labels, const int64_t* set_ptr, const int32_t* set_nodes,
                                      int64_t n_sets, float* out, int32_t* out_status, void* workspace, int64_t workspace_bytes,
                                      void* stream);

/* ---------------------------------------------------------------------------------------
 * a11  Structure similarity: 1 / (1 + fastdtw(x, y, radius=1, dist=calc_dist)).
 * Replaces gamma.calc_dist / gamma.calc_dtw (SubGNN/gamma.py:51-59) and the all-pairs driver
 * SubGNN.compute_structure_patch_similarities (SubGNN/SubGNN.py:783-833).
 * x = CC degree sequences (x_ptr/x_val, n_x rows), y = anchor degree sequences (n_y rows);
 * out (n_x, n_y) float32; rows with an empty x are PAD (SubGNN.py:831).  fp64 DP.
 * tie_order 0 = (i-1,j),(i,j-1),(i-1,j-1) first minimum (pure-Python fastdtw 0.3.4).
 * x_order (nullable, int32[n_x], a permutation): processing order of the x rows -- results are
 * unaffected; putting similar rows next to each other keeps a wavefront's lanes in step.
 * workspace: sgnn_dtw_workspace_bytes(n_x, max_x_len, n_y, max_y_len) bytes (any content).
 * ------------------------------------------------------------------------------------- */
/* Keys whose ascending order is a good processing order (x_order) for sgnn_dtw_similarity: (length, up to six
 * entries of the row's twice-halved series on a log scale), packed into an int64 per x row; empty rows sort first.
 * Sorting by them is the caller's (any sort). */
int sgnn_dtw_order_keys(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t* out_keys, void* stream);
int64_t sgnn_dtw_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len);
/* kernel: 0 = pick by size (x rows of at most 32 entries: the register-resident kernel), 1 = the general
 * (workspace-resident) kernel whatever the size -- same values, bit for bit */
int sgnn_dtw_similarity(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                        const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                        int tie_order, int kernel, const int32_t* x_order, float* out, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Same, for callers whose x rows are mostly empty (repeated rows given length 0 by a grouping step):
 * x_live_range (device, int64[2] = {first, count}, nullable) names the positions of the processing
 * order x_order that hold the non-empty rows -- x_order must list the empty rows first -- and only those
 * are computed; the caller zero-fills (PAD) the output beforehand.  The range lives on the device so
 * that no host round trip is needed to learn it. */
int sgnn_dtw_similarity_live(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                             const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                             int tie_order, int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* The x side prepared ONCE, for a caller whose x rows hold the same values from call to call (the degree sequences of a
 * split's components): sgnn_dtw_prepare_rows writes the value and reciprocal pyramids and the lengths of the x rows --
 * what sgnn_dtw_similarity builds into its workspace on every call -- into ``rows``, a device buffer of
 * sgnn_dtw_rows_bytes(n_x, max_x_len) bytes that the caller owns and keeps alive, and describes it in ``header``, HOST
 * memory of sgnn_dtw_rows_header_words() int64 that the caller keeps with it (magic, layout, n_x, max_x_len, the buffer's
 * address and size).  The layout is the one the kernel picked by (max_x_len, kernel, x_order) reads: the register kernel's
 * (positions follow x_order) or the general kernel's (positions are the row numbers).
 * sgnn_dtw_similarity_rows / _rows_live are sgnn_dtw_similarity / _live without the x pyramid launch: they take the header
 * instead of x_ptr / x_val, with the SAME n_x, max_x_len, kernel and x_order (the same permutation) as the preparation; a
 * header that was not filled by sgnn_dtw_prepare_rows, or for another row count, length bound or layout, is
 * SGNN_ERR_BAD_ARG -- nothing is launched.  Their workspace (sgnn_dtw_rows_workspace_bytes) does not hold the x pyramids.
 * Same values as sgnn_dtw_similarity, bit for bit (the same kernels read the same pyramids). */
int64_t sgnn_dtw_rows_bytes(int64_t n_x, int64_t max_x_len);
int64_t sgnn_dtw_rows_header_words(void);
int64_t sgnn_dtw_rows_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len);
int sgnn_dtw_prepare_rows(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len, int kernel,
                          const int32_t* x_order, void* rows, int64_t rows_bytes, int64_t* header, void* stream);
int sgnn_dtw_similarity_rows(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                             const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                             int tie_order, int kernel, const int32_t* x_order, float* out, void* workspace,
                             int64_t workspace_bytes, void* stream);
int sgnn_dtw_similarity_rows_live(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                                  const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                  int tie_order, int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a11x Structure similarity with the EXACT distance: 1 / (1 + DTW(x, y, dist=calc_dist)), the minimum over all warp
 * paths of the whole grid -- what fastdtw approximates (hparams['structure_similarity_fn'] = 'dtw_exact').
 *   D[i][j] = min(D[i-1][j], D[i][j-1], D[i-1][j-1]) + calc_dist(x[i], y[j])
 * The value does not depend on a predecessor rule, so there is no tie_order.  Everything else is as for
 * sgnn_dtw_similarity: same x / y / out conventions, fp64 DP, out = float(1 / (1 + d)), rows with an empty x are PAD, and
 * so is every pair of an empty y row (what sgnn_dtw_similarity writes for one); x_order and x_live_range mean the same.
 * kernel: 0 = pick by size (x rows of at most 32 entries: the register-resident kernel), 1 = the general kernel (the
 * lane's column in the workspace) whatever the size -- same values, bit for bit.
 * workspace: sgnn_dtw_exact_workspace_bytes(n_x, max_x_len, n_y, max_y_len) bytes (any content).
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_dtw_exact_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len);
int sgnn_dtw_exact_similarity(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                              const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                              int kernel, const int32_t* x_order, float* out, void* workspace,
                              int64_t workspace_bytes, void* stream);
int sgnn_dtw_exact_similarity_live(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len,
                                   const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                   int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                                   void* workspace, int64_t workspace_bytes, void* stream);
/* The x side (value + 1, reciprocals, lengths) prepared once: as sgnn_dtw_prepare_rows / sgnn_dtw_similarity_rows above, with
 * the same header form (sgnn_dtw_rows_header_words() words) and a magic of its own -- a buffer of one is refused by the other. */
int64_t sgnn_dtwx_rows_bytes(int64_t n_x, int64_t max_x_len);
int64_t sgnn_dtwx_rows_workspace_bytes(int64_t n_x, int64_t max_x_len, int64_t n_y, int64_t max_y_len);
int sgnn_dtwx_prepare_rows(const int64_t* x_ptr, const int32_t* x_val, int64_t n_x, int64_t max_x_len, int kernel,
                                const int32_t* x_order, void* rows, int64_t rows_bytes, int64_t* header, void* stream);
int sgnn_dtwx_similarity_rows(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                                   const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                   int kernel, const int32_t* x_order, float* out, void* workspace,
                                   int64_t workspace_bytes, void* stream);
int sgnn_dtwx_similarity_rows_live(const int64_t* rows_header, int64_t n_x, int64_t max_x_len,
                                        const int64_t* y_ptr, const int32_t* y_val, int64_t n_y, int64_t max_y_len,
                                        int kernel, const int32_t* x_order, const int64_t* x_live_range, float* out,
                                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * n1   Nearest rows of a bank of embeddings: the best k of every query's scores, without the Q x N score matrix.
 * Replaces no reference function (the reference stops at the subgraph embeddings; subgnn_amd/neighbors.py compares them).
 *   q (Q, D) and bank (N, D) float32, row-major with row strides q_stride / b_stride >= D (in elements); D >= 1, Q >= 1,
 *   0 <= N < 2^31 (N == 0: bank may be NULL).
 *   dot(i, j) = the float32 chain acc = fmaf(q[i][d], bank[j][d], acc), d = 0 .. D-1 ascending, from acc = 0
 *               (v_mfma_f32_32x32x2_f32; tails are padded with zeros, and fmaf(0, 0, acc) == acc)
 *   SGNN_TOPK_DOT     score = dot                                   higher is better
 *   SGNN_TOPK_COSINE  score = (dot * q_aux[i]) * b_aux[j]           higher is better; aux = the caller's inverse norms
 *   SGNN_TOPK_L2      score = (q_aux[i] + b_aux[j]) - 2 * dot       lower is better;  aux = the caller's squared norms
 *   each operation rounded once, as written.  q_aux (Q) / b_aux (N) float32: required for cosine and l2, ignored for dot.
 * Order: strict and total -- the better score first, equal scores (-0 == +0) by the smaller bank row, a NaN score behind
 * every number (by row again).  exclude (Q) int64, nullable: a bank row that query skips, or -1.  Row i of out_score (Q, k)
 * float32 / out_index (Q, k) int64 lists the first k of that order, best first; slots beyond the candidates hold index -1 and
 * score -inf (+inf for l2).  A zero score is returned as +0 and a NaN as the quiet NaN 0x7FC00000.  The result does not depend
 * on `splits`, the number of bank slices that are searched apart and merged: 0 = the library chooses, 1 .. 1024 = as given.
 * 1 <= k <= sgnn_topk_max_k() (64).  Anything else -- a bad metric, a missing aux vector, a NULL q or output, Q or D < 1, a
 * workspace smaller than sgnn_topk_rows_workspace_bytes(Q, N, k, splits) (which may be 0: workspace NULL is fine then; < 0
 * for arguments the call would refuse) -- returns SGNN_ERR_BAD_ARG and writes nothing.  No float atomics; deterministic.
 * ------------------------------------------------------------------------------------- */
#define SGNN_TOPK_DOT    0
#define SGNN_TOPK_COSINE 1
#define SGNN_TOPK_L2     2
int64_t sgnn_topk_max_k(void);
int64_t sgnn_topk_rows_workspace_bytes(int64_t Q, int64_t N, int64_t k, int64_t splits);
int sgnn_topk_rows(const float* q, int64_t q_stride, int64_t Q, const float* bank, int64_t b_stride, int64_t N,
                   int64_t D, int64_t k, int metric, const float* q_aux, const float* b_aux, const int64_t* exclude,
                   int64_t splits, float* out_score, int64_t* out_index, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* ---------------------------------------------------------------------------------------
 * n2   k-means over a bank of embeddings: one Lloyd iteration = sgnn_kmeans_step + sgnn_kmeans_finish, no (N, K) matrix,
 * no atomics on floats, nothing returned to the host.  Replaces no reference function.
 *   x (N, D) and c (K, D) float32, row-major with row strides x_stride / c_stride >= D (in elements); x_aux (N) / c_aux (K)
 *   the vectors sgnn_topk_rows takes beside them.  metric: SGNN_TOPK_L2 (k-means) or SGNN_TOPK_COSINE (spherical k-means on
 *   rows the caller has normalised); SGNN_TOPK_DOT is refused.
 * sgnn_kmeans_step
 *   assign[i] (int32) / score[i]: exactly index and score of sgnn_topk_rows(x, c, k = 1, metric, x_aux, c_aux) -- the same
 *   fmaf chain, epilogue and total order (better score, then the smaller centre, NaN last), for every grid.
 *   The rows are dealt to S = sgnn_kmeans_slots(N, K, D) workgroups as contiguous ranges of 32-row tiles:
 *   S = min(ceil(N / 32), 1024, max(1, 64 MiB / (4 K D))), then evened so that no slot is empty.  Slot s leaves in the
 *   workspace: per cluster the float32 chain acc = acc + x[i][d] from +0 over its rows of the cluster in ascending i; the
 *   rows' count; the number of its rows with assign[i] != prev_assign[i] (prev_assign NULL: all of them; it must not be the
 *   array `assign`); and the double sum of its scores -- per 32-row tile the butterfly t[r] += t[r ^ 16], ^ 8, ^ 4, ^ 2, ^ 1
 *   (rows past N count 0), the tiles added in ascending order.
 * sgnn_kmeans_finish (same N, K, D, metric and workspace; c = the centres the step used)
 *   sums (K, D) = the chain acc = acc + partial over the slots in slot order from +0; counts (K) int32; *inertia (double)
 *   and changed[it] (int32; `it` >= 0 indexes a device array, so a loop of iterations needs no read-back) the slots' sums in
 *   slot order; c_next (K, D, contiguous; may be c itself) = sums / (float)counts, one correctly rounded division, or the
 *   row of c for a cluster without rows; *empty (int32) the number of such clusters; c_aux_next (K): with
 *   q = the chain fmaf(v, v, q) of thread t over d = t, t + 256, ... and then q[t] += q[t + 128], q[t + 64], ..., q[t + 1],
 *   q[0] for l2 and 1 / sqrt(max(q[0], 1e-30)) (both correctly rounded) for cosine.
 * Limits: 1 <= K <= sgnn_kmeans_max_k() (1024); 1 <= N < 2^31 - 256; 1 <= D; strides < 2^23 (topk_rows' limits); float32.
 * Anything else -- a refused metric, a NULL array other than prev_assign, a workspace smaller than
 * sgnn_kmeans_workspace_bytes(N, K, D) (< 0 for sizes the calls refuse) -- returns SGNN_ERR_BAD_ARG before any launch, with
 * nothing written.  A call repeats bit for bit; a step whose assignment equals prev_assign's yields the same c_next bits.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_kmeans_max_k(void);
int64_t sgnn_kmeans_slots(int64_t N, int64_t K, int64_t D);
int64_t sgnn_kmeans_workspace_bytes(int64_t N, int64_t K, int64_t D);
int sgnn_kmeans_step(const float* x, int64_t x_stride, int64_t N, const float* c, int64_t c_stride, int64_t K, int64_t D,
                     int metric, const float* x_aux, const float* c_aux, const int32_t* prev_assign, int32_t* assign,
                     float* score, void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_kmeans_finish(const void* workspace, int64_t workspace_bytes, int64_t N, int64_t K, int64_t D, int metric,
                       const float* c, int64_t c_stride, float* sums, int32_t* counts, double* inertia, int32_t* empty,
                       float* c_next, float* c_aux_next, int32_t* changed, int64_t it, void* stream);

/* ---------------------------------------------------------------------------------------
 * a12  CC embedding initialisation: sum or max of member node embeddings.
 * Replaces SubGNN.initialize_cc_embeddings (SubGNN/SubGNN.py:609-622).  E: (n_emb_rows, D) f32.
 * aggregator 0 = sum, 1 = max.  For max, a row shorter than padded_len also competes with the
 * zero PAD row (SubGNN.py:622); out_arg (n_sets, D) int32 receives the winning node id
 * (0 = PAD) for the backward pass.
 * ------------------------------------------------------------------------------------- */
int sgnn_cc_embed_fwd(const float* E, int64_t D,
                      const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                      int aggregator, int64_t padded_len, float* out, int32_t* out_arg, void* stream);
/* same with the table stored as IEEE half (rows, D): read as half, accumulated and returned in fp32
 * (BASELINE.json configs[4]: "fp16 embeddings"); the backward is sgnn_cc_embed_bwd (fp32 gradient). */
int sgnn_cc_embed_fwd_f16(const uint16_t* E_half, int64_t D,
                          const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                          int aggregator, int64_t padded_len, float* out, int32_t* out_arg, void* stream);
/* grad_E (n_emb_rows, D) is accumulated into (float atomics), row PAD untouched */
int sgnn_cc_embed_bwd(const float* grad_out, int64_t D,
                      const int64_t* set_ptr, const int32_t* set_nodes, int64_t n_sets,
                      int aggregator, const int32_t* arg, float* grad_E, void* stream);

/* ---------------------------------------------------------------------------------------
 * a13+a15  One anchor -> component message-passing layer (gather, weight, aggregate, read-out).
 * Replaces the body of SG_MPN.forward / propagate / message / generate_pos_struc_embeddings
 * (SubGNN/subgraph_mpn.py:105-174, 227-231) together with the anchor gather of
 * anchor_patch_samplers.get_anchor_patches / embed_anchor_patch (anchor_patch_samplers.py:
 * 333-411).  For row r (= b*C + c) and anchor slot a:
 *     edge(r,a)  -- see `src`
 *     w          = sims[r*sims_ld + column(r,a)]
 *     agg[r,:]   = sum_a edge * w * x(r,a,:)
 *     z[r,a]     = edge ? w * <wp, x(r,a,:)> + bp : bp       (pre-activation read-out)
 * Anchor rows x(r,a,:) come from one of three sources:
 *   SGNN_SRC_DENSE  x = anchor_embeds[(r*A+a)*D ..]  (the reference's materialised (B,C,A,D)
 *                   tensor); edge = edge_mask[r*A+a]
 *   SGNN_SRC_GATHER x = E[ids[(r/id_div)*A+a]*D ..]; edge = id != 0 && row_mask[r]
 *   SGNN_SRC_SHARED x = X[a*D ..] (P-border / structure anchors shared by every row);
 *                   edge = row_mask[r] && (ids == NULL || ids[a] != 0)
 * column(r,a): sim_col != NULL -> sim_col[a]; else sims_per_edge -> a; else id - 1.
 * The Linear(2D->D)+ReLU update (subgraph_mpn.py:233-239) is a plain GEMM done by the caller.
 * ------------------------------------------------------------------------------------- */
#define SGNN_SRC_DENSE  0
#define SGNN_SRC_GATHER 1
#define SGNN_SRC_SHARED 2

typedef struct sgnn_mpn_args {
    int32_t src;               /* SGNN_SRC_* */
    int32_t sims_per_edge;     /* 1: sims is (R, A) already gathered */
    int64_t R, A, D;
    const float*   x;          /* DENSE: (R,A,D) anchor_embeds; GATHER: E (rows,D); SHARED: X (A,D) */
    const int64_t* ids;        /* DENSE/GATHER: (R/id_div, A) anchor ids; SHARED: (A) or NULL */
    int64_t        id_div;     /* rows sharing one ids row (C for P-internal, else 1) */
    const uint8_t* edge_mask;  /* DENSE: (R,A) */
    const uint8_t* row_mask;   /* GATHER/SHARED: (R) cc_embed_mask, may be NULL (= all real) */
    const float*   sims;       /* (R, sims_ld) */
    int64_t        sims_ld;
    const int64_t* sim_col;    /* (A) or NULL */
    const float*   wp;         /* (D) linear_position.weight */
    const float*   bp;         /* (1) linear_position.bias   */
    int32_t        x_f16;      /* GATHER only: x points at an IEEE half table (rows, D), read as
                                * half and accumulated in fp32 (gradients stay fp32) */
    const float*   z_act;      /* nullable, (R, A): the read-out as sgnn_mpn_fwd wrote it under SGNN_MPN_RELU_Z.  When set, every
                                * backward entry point takes grad_z through that relu: an entry whose z_act is not > 0 counts as 0 */
    int32_t        flags;      /* SGNN_MPN_WP_PARTIAL: sgnn_mpn_bwd (DENSE) writes grad_wp as per-row partial sums (R, D)
                                * for the caller to add up in a fixed order, instead of adding into (D) with atomics.
                                * SGNN_MPN_RELU_Z: sgnn_mpn_fwd writes the read-out AFTER its non-linearity, relu(z) (mpn:122-131
                                * generate_pos_struc_embeddings applies it next), instead of the pre-activation */
} sgnn_mpn_args;
#define SGNN_MPN_WP_PARTIAL 1
#define SGNN_MPN_RELU_Z     2

/* Batch-sized calls (a few hundred rows) split the anchors of a row over sgnn_mpn_fwd_chunks(args) chunks so that
 * the launch fills the chip; chunk c writes its partial aggregate to agg + c * R * D and the caller adds the
 * chunks up (a fixed order: no atomics).  agg: (chunks, R, D); 1 chunk for shard-sized calls. */
int sgnn_mpn_fwd_chunks(const sgnn_mpn_args* args);
int sgnn_mpn_fwd(const sgnn_mpn_args* args, float* agg /*(chunks,R,D)*/, float* z /*(R,A)*/, void* stream);
/* The bodies of ONE message-passing layer (up to sgnn_mpn_fwd_many_max_bodies(): they read the layer below only) in one launch:
 * args is a HOST array of n argument blocks, agg[k] / z[k] (HOST arrays of DEVICE pointers) as sgnn_mpn_fwd writes them for
 * args[k] (agg[k]: sgnn_mpn_fwd_chunks(&args[k]) chunks; z[k] nullable).  Every body needs R > 0 and A > 0. */
int64_t sgnn_mpn_fwd_many_max_bodies(void);
int sgnn_mpn_fwd_many(int64_t n, const sgnn_mpn_args* args, float* const* agg, float* const* z, void* stream);
/* grad_x: DENSE (R,A,D) written; GATHER (rows,D) accumulated with float atomics, row PAD
 * untouched (the atomics-free form of GATHER: sgnn_mpn_bwd_edges + sgnn_scatter_add_rows_sorted); SHARED (A,D)
 * accumulated.  grad_wp (D) accumulated, or (R,D) written with SGNN_MPN_WP_PARTIAL.  Any of them may be NULL. */
int sgnn_mpn_bwd(const sgnn_mpn_args* args, const float* grad_agg, const float* grad_z,
                 float* grad_x, float* grad_wp, void* stream);

/* ---------------------------------------------------------------------------------------
 * a16 (optional ff_attn read-out)  Additive-attention scores over a subgraph's components.
 * Replaces attention.AdditiveAttention._forward_internal (SubGNN/attention.py:130-139) as used at
 * SubGNN/SubGNN.py:298-301:  out[r] = sum_j v[j] * tanh(qW[r / rows_per_batch, j] + (X U)[r, j]).
 * X (R, H) component embeddings, U (H, H) = _u_matrix, qW (R / rows_per_batch, H) = vector @ _w_matrix,
 * v (H) = _v_vector.
 * ------------------------------------------------------------------------------------- */
/* exact f32 form: the caller's BLAS computes XU = X U (a plain dense GEMM); this is everything after it, fused:
 * out[r] = sum_j v_j tanh(XU[r, j] + qW[r / rows_per_batch, j]). */
int sgnn_attn_scores_epilogue(const float* XU, const float* qW, const float* v, int64_t R, int64_t H,
                              int64_t rows_per_batch, float* out, void* stream);
/* half operands on the matrix cores, one kernel (v_mfma_f32_32x32x16_f16, fp32 accumulate; X and U are rounded to IEEE
 * half on the way in; four wavefronts per workgroup share each 32-column panel of U through LDS): the fp16 form of
 * BASELINE.json configs[4].  H <= 640, else SGNN_ERR_UNSUPPORTED_D (the caller takes the exact form).
 * workspace: sgnn_attn_scores_f16_workspace_bytes(H) bytes (the transposed half copy of U). */
int64_t sgnn_attn_scores_f16_workspace_bytes(int64_t H);
int sgnn_attn_scores_fwd_f16(const float* X, const float* U, const float* qW, const float* v,
                             int64_t R, int64_t H, int64_t rows_per_batch, float* out,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a14 (walk aggregator)  The recurrence of one bidirectional LSTM layer, whole sequence per launch.
 * Replaces the nn.LSTM(bidirectional=True, batch_first=True) inside the reference's LSTM module
 * (SubGNN/SubGNN.py:60-88) as called by aggregate_structure_anchor_patch
 * (SubGNN/anchor_patch_samplers.py:413-433) on (patches x walks, walk_len, D).  h0 = c0 = 0.
 * The non-recurrent contractions are plain GEMMs over all (sequence, step) rows and stay with the
 * caller's BLAS: the input projection before the forward call, dx / dW_ih / dW_hh / db after the
 * backward call.  Gate order i, f, g, o (torch).
 *   pre_x  (2, B, T, 4H)   x W_ih^T + b_ih per direction (0 = forward, 1 = reverse), direction-major: each direction's
 *                          rows are one GEMM's contiguous output
 *   whh_f, whh_r (4H, H)   weight_hh per direction;  bhh_f, bhh_r (4H), nullable: bias_hh per direction, added here (the
 *                          caller needs no concatenated weights and no summed biases: five small launches per layer less)
 *   y      (B, T, 2H)      [forward h_t | reverse h_t]  (torch's output layout)
 *   gates  (2, B, T, 4H), cell (2, B, T, H), hprev (2, B, T, H) = h_{t-1} in the direction's order:
 *          activations kept for the backward pass
 * backward: dy (B, T, 2H) -> dgates (2, B, T, 4H), the gradient w.r.t. pre_x.  Then, with dG[d] = dgates[d] viewed (B T, 4H):
 * dx = dG[0] W_ih_f + dG[1] W_ih_r,  dW_ih[d] = dG[d]^T x,  dW_hh[d] = dG[d]^T hprev[d],  db[d] = column sums of dG[d].
 * Hidden sizes 32, 64, 128 (sgnn_lstm_supported), any input size; else SGNN_ERR_UNSUPPORTED_D -- the
 * caller keeps the library LSTM for those.
 * ------------------------------------------------------------------------------------- */
int sgnn_lstm_supported(int64_t hidden_size);
int sgnn_lstm_fwd(const float* pre_x, const float* whh_f, const float* whh_r, const float* bhh_f, const float* bhh_r,
                  int64_t B, int64_t T, int64_t hidden_size, float* y, float* gates, float* cell, float* hprev, void* stream);
int sgnn_lstm_bwd(const float* whh_f, const float* whh_r, const float* gates, const float* cell, const float* dy,
                  int64_t B, int64_t T, int64_t hidden_size, float* dgates, void* stream);

/* The dense products around the recurrence, and the walk aggregator's tail (anchor_patch_samplers.py:413-433 / SubGNN.py:60-88:
 * embedding lookup -> LSTM -> last step (or sum over steps) -> Linear -> sum over a patch's walks), in this library's launches:
 *   sgnn_rows_gemm     out[z] (R, N) = X[row(r)] W_z^T + b_z for z = 0 (and 1 when W1 is given): fp32 MFMA; row(r) = ids[r] when
 *                      ids (int64, nullable) is given -- the gather of the input rows is the operand load -- and the gathered
 *                      rows are written to x_copy (R, K; nullable).  X rows of ldx floats, K % 8 == 0; W_z (N, K) row-major.
 *   sgnn_rows_gemm_nt  out (R, N) = A[0] W0 + A[1] W1 with A (2, R, K) and W_z (K, N) row-major (dx of both directions).
 *   sgnn_lstm_tail_fwd X (n_patches, D) = s W_lin^T + n_walks b_lin, s[p] = sum over the patch's walks of y[walk][T - 1] (last_only)
 *                      or of every step; y (n_patches n_walks, T, H2); s_out (n_patches, H2) kept for the backward.
 *   sgnn_lstm_tail_bwd dy (same shape as y, every element written), dW_lin (D, H2), db_lin (D) (both nullable) from dX and s. */
int sgnn_rows_gemm(const float* X, const int64_t* ids, int64_t ldx, int64_t R, int64_t K, const float* W0, const float* W1,
                   const float* b0, const float* b1, int64_t N, float* out, float* x_copy, void* stream);
int sgnn_rows_gemm_nt(const float* A, int64_t R, int64_t K, const float* W0, const float* W1, int64_t N, float* out, void* stream);
int sgnn_lstm_tail_fwd(const float* y, int64_t n_patches, int64_t n_walks, int64_t T, int64_t H2, int last_only,
                       const float* W_lin, const float* b_lin, int64_t D, float* s_out, float* X, void* stream);
int sgnn_lstm_tail_bwd(const float* dX, const float* s, int64_t n_patches, int64_t n_walks, int64_t T, int64_t H2,
                       int last_only, const float* W_lin, int64_t D, float* dy, float* dW_lin, float* db_lin, void* stream);

/* ---------------------------------------------------------------------------------------
 * a16  The tail of the forward pass without the (B, C, H) concatenation (SubGNN/SubGNN.py:286-312: cat of the
 * channel outputs, then masked_sum): every piece is summed over a subgraph's real components straight into its
 * column slot of the (B, H) subgraph embedding (row stride out_ld / grad_ld, in floats).
 *   sgnn_masked_sum_slot_fwd/_bwd: a piece that exists as a tensor x (B, C, W) (component embeddings), mask (B, C):
 *     the masked sum over the components of a subgraph (subgraph_utils.masked_sum, SubGNN/subgraph_utils.py:213-237,
 *     as used at SubGNN/SubGNN.py:303) into columns [0, W) of out; backward scatters those columns of grad_out to
 *     the real components.  out_ld == W (grad_ld == W) is the plain masked sum x (B, C, W) -> out (B, W).
 *   sgnn_readout_many_fwd/_bwd (below): the read-outs of layers over SHARED anchors, of which only the sum is consumed.
 * ------------------------------------------------------------------------------------- */
int sgnn_masked_sum_slot_fwd(const float* x, const uint8_t* mask, int64_t B, int64_t C, int64_t W, float* out,
                             int64_t out_ld, void* stream);
int sgnn_masked_sum_slot_bwd(const float* grad_out, int64_t grad_ld, const uint8_t* mask, int64_t B, int64_t C,
                             int64_t W, float* grad_x, void* stream);
/* The same for n_pieces tensors in one launch (per 96 pieces): xs[i] (B, C, widths[i]) summed into columns
 * [offsets[i], offsets[i] + widths[i]) of out (B, out_ld); backward: grad_xs[i] (B, C, widths[i]) written from those columns of
 * grad_out (a null grad_xs[i] is skipped).  xs / grad_xs / widths / offsets are HOST arrays (of DEVICE pointers).  The form a
 * batch-sized step uses: 22 pieces of a 4-layer model are one launch each way instead of 22. */
int sgnn_masked_sum_slots_fwd(const float* const* xs, const int64_t* widths, const int64_t* offsets, int64_t n_pieces,
                              const uint8_t* mask, int64_t B, int64_t C, float* out, int64_t out_ld, void* stream);
int sgnn_masked_sum_slots_bwd(const float* grad_out, int64_t grad_ld, const uint8_t* mask, int64_t B, int64_t C,
                              float* const* grad_xs, const int64_t* widths, const int64_t* offsets, int64_t n_pieces, void* stream);

/* ---------------------------------------------------------------------------------------
 * a17  Loss + accuracy of a step: nn.CrossEntropyLoss() with its default mean reduction (SubGNN/SubGNN.py:133, applied
 * at SubGNN.py:1116-1124) and subgraph_utils.calc_accuracy (SubGNN/subgraph_utils.py:108-124: argmax == label, mean)
 * in one pass over logits (B, K) row-major, labels int64 (B) in [0, K) or -100 (nn.CrossEntropyLoss's ignore_index: the row
 * contributes nothing and the mean is over the other rows; any other label outside [0, K) makes the loss NaN -- the library
 * raises).  lse (B + 1 floats): the rows' log-sum-exp and, in lse[B], the number of rows not ignored, kept for the
 * backward.  loss, accuracy: one float each (accuracy nullable; over all B rows).
 * grad_logits = (softmax - onehot) * grad_loss[0] / lse[B].
 * Partial sums are added in a fixed order: bit-reproducible.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_cross_entropy_workspace_bytes(int64_t B);
int sgnn_cross_entropy_fwd(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                           float* accuracy, void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_cross_entropy_bwd(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss,
                           int64_t B, int64_t K, float* grad_logits, void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-label loss and accuracy of a training step in one pass over the logits: nn.BCEWithLogitsLoss() (mean over all B x K
 * elements, SubGNN/SubGNN.py:133) and the exact-match accuracy the step logs (subgraph_utils.calc_accuracy with a binarizer,
 * SubGNN/subgraph_utils.py:108-124: a row counts when sigmoid(x) > 0.5 equals the target in every column).
 * logits: (B, K) float, targets: (B, K) int64 indicator matrix (non-zero counts as 1), any K.  loss, accuracy: one float each
 * (accuracy nullable).  The prediction is the float32 expression 1 / (1 + exp(-x)) > 0.5, as torch.sigmoid(x) > 0.5.
 * grad_logits = (sigmoid(x) - y) * grad_loss[0] / (B K), the sigmoid evaluated without overflow.  Nothing is saved between the
 * two calls.  workspace: sgnn_bce_logits_workspace_bytes(B) bytes.  Partial sums are added in a fixed order: bit-reproducible.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_bce_logits_workspace_bytes(int64_t B);
int sgnn_bce_logits_fwd(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                        void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_bce_logits_bwd(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                        float* grad_logits, void* stream);

/* ---------------------------------------------------------------------------------------
 * The two pairs above with class weights: torch's `weight` of nn.CrossEntropyLoss and `weight` / `pos_weight` of
 * nn.BCEWithLogitsLoss, the two loss modules built at SubGNN/SubGNN.py:133 (mean reduction).  The argument lists are those of
 * the bare entries plus the weight rows at the end: DEVICE pointers to K floats each, nullable -- with every row null the call IS
 * the bare entry (the same kernel).  The bare entries forward here with nulls.
 *   single-label   loss = sum_i w[y_i] (lse_i - x[i, y_i]) / sum_i w[y_i] over the rows with y_i != -100;
 *                  grad_logits[i, :] = w[y_i] (softmax_i - onehot(y_i)) grad_loss[0] / lse[B]; lse[B] = sum_i w[y_i], the divisor
 *                  (0 gives NaN, as torch does).  A label outside [0, K) other than -100 makes the loss NaN as before, and
 *                  w[y] is never read for it.  The accuracy stays unweighted, over all B rows.
 *   multi-label    with y in {0, 1}, c = weight, p = pos_weight, L = 1 + (p_k - 1) y: element loss
 *                  c_k [(1 - y) x + L (log1p(exp(-|x|)) + max(-x, 0))], mean over B K;
 *                  grad_logits = c_k [(1 - y) - L (1 - sigmoid(x))] grad_loss[0] / (B K), evaluated without overflow.
 * Workspaces, partials and the fixed summation order are those of the bare entries: bit-reproducible.
 * ------------------------------------------------------------------------------------- */
int sgnn_cross_entropy_fwd_weighted(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                                    float* accuracy, void* workspace, int64_t workspace_bytes, void* stream,
                                    const float* class_weight);
int sgnn_cross_entropy_bwd_weighted(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss,
                                    int64_t B, int64_t K, float* grad_logits, void* stream, const float* class_weight);
int sgnn_bce_logits_fwd_weighted(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                                 void* workspace, int64_t workspace_bytes, void* stream, const float* weight,
                                 const float* pos_weight);
int sgnn_bce_logits_bwd_weighted(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                                 float* grad_logits, void* stream, const float* weight, const float* pos_weight);

/* Shaped losses: label smoothing and focal loss on the two pairs above.  The argument lists are those of the _weighted entries
 * plus `float label_smoothing, float focal_gamma` (the bce entries: focal_gamma only).  With both 0 the call IS the _weighted
 * entry (and with null rows the bare one).  label_smoothing outside [0, 1), a negative or non-finite focal_gamma, or both
 * non-zero: SGNN_ERR_BAD_ARG before any launch, nothing is written.  Otherwise kernels of their own run; an absent weight row
 * stands as ones.  With w the class weights (W their sum), p = softmax(x_i), y the label, D = sum_i w[y_i] over counted rows:
 *   smoothing eps  (F.cross_entropy(weight=, label_smoothing=), mean)
 *                  loss = sum_i [(1 - eps) w_y (lse_i - x_iy) + (eps / K) sum_k w_k (lse_i - x_ik)] / D;
 *                  grad_logits[i, k] = [(1 - eps) w_y (p_k - [k == y]) + (eps / K) (W p_k - w_k)] grad_loss[0] / D
 *   focal gamma    lp = x_iy - lse_i, p_t = exp(lp), q = -expm1(lp): loss = sum_i w_y q^gamma (-lp) / D;
 *                  grad_logits[i, k] = w_y f_i (p_k - [k == y]) grad_loss[0] / D, f_i = q^gamma - gamma p_t q^(gamma - 1) lp;
 *                  a row with q = 0 has loss and f_i exactly 0
 *   focal gamma, multi-label   s = +1 for a target, -1 otherwise, z = s x, e = exp(-|z|), l = log1p(e) + max(-z, 0),
 *                  q = sigmoid(-z), p_t = sigmoid(z) (both from e), c = weight_k, L = pos_weight_k for a target, else 1:
 *                  element loss c L q^gamma l, mean over B K; grad_logits = -s c L q^gamma (q + gamma p_t l) grad_loss[0] / (B K)
 * lse[B] stays the divisor D; labels of -100 are ignored and any other label outside [0, K) makes the loss NaN, as before;
 * the accuracy is unweighted and unchanged.  Workspaces, partials and summation orders are the bare entries': bit-reproducible. */
int sgnn_cross_entropy_fwd_shaped(const float* logits, const int64_t* labels, int64_t B, int64_t K, float* lse, float* loss,
                                  float* accuracy, void* workspace, int64_t workspace_bytes, void* stream,
                                  const float* class_weight, float label_smoothing, float focal_gamma);
int sgnn_cross_entropy_bwd_shaped(const float* logits, const int64_t* labels, const float* lse, const float* grad_loss,
                                  int64_t B, int64_t K, float* grad_logits, void* stream, const float* class_weight,
                                  float label_smoothing, float focal_gamma);
int sgnn_bce_logits_fwd_shaped(const float* logits, const int64_t* targets, int64_t B, int64_t K, float* loss, float* accuracy,
                               void* workspace, int64_t workspace_bytes, void* stream, const float* weight,
                               const float* pos_weight, float focal_gamma);
int sgnn_bce_logits_bwd_shaped(const float* logits, const int64_t* targets, const float* grad_loss, int64_t B, int64_t K,
                               float* grad_logits, void* stream, const float* weight, const float* pos_weight, float focal_gamma);

/* Column sums of a row-major matrix x (R rows of A floats, row stride ld): out[a] = sum_r x[r, a] -- the bias gradients of the
 * head's Linear layers over a shard's rows (autograd of SubGNN/SubGNN.py:304-312).  Row-block partials added in block order:
 * bit-reproducible.  workspace: sgnn_column_sum_workspace_bytes. */
int64_t sgnn_column_sum_workspace_bytes(int64_t R, int64_t A);
int sgnn_column_sum(const float* x, int64_t ld, int64_t R, int64_t A, float* out, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* The read-out of a layer over SHARED anchors (subgraph_mpn.py:122-131: position read-out of the messages + relu) when only
 * its sum over a subgraph's components is consumed: with the scores s[a] = X[a, :] . wp
 *     out[b, off + a] = sum over real components c of  relu(W[b,c,a] * s[a] + bp[0]),
 *     W[b,c,a] = sims[(b C + c) sims_ld + (sim_col ? sim_col[a] : a)]    (sims NULL: W = 0)
 * for every read-out piece of a step in ONE launch each way (n <= sgnn_readout_many_max() pieces; all arrays HOST arrays with
 * one entry per piece, of DEVICE pointers where they hold pointers).  Piece k: similarity rows sims[k] (ld sims_ld[k]; NULL = all
 * zero), columns sim_col[k] (nullable), anchor embeddings X[k] (A[k], D) with read-out weight wp[k] (D) -- the scores, 0 where
 * ids[k][a] == 0 (ids nullable) or X[k] is NULL, are computed by the call into s[k] (A[k] floats) --
 * bias bp[k], row mask row_mask[k] (B C, nullable: 0 = padded component, contributes nothing), column slot off[k] .. off[k] + A[k]
 * of the (B, out_ld) embedding.  Backward: d s[a] = sum_r g [z>0] W and grad_bp = sum g [z>0] by per-row-block partials added in
 * block order (no atomics on a value: bit-reproducible), grad_X[k] (A[k], D) = d s wp^T, grad_wp[k] (D) = X^T d s, grad_bp[k] (1),
 * each nullable; tickets: RO_MAX_PIECES uint32, zero before the first call and left zero.  Scores that exist already go in as
 * X (A, 1) with wp = {1}: s is X exactly and grad_X is d s. */
int64_t sgnn_readout_many_max(void);
int sgnn_readout_many_fwd(int64_t n, const float* const* sims, const int64_t* sims_ld, const int64_t* const* sim_col,
                          const float* const* X, const float* const* wp, const float* const* bp,
                          const int64_t* const* ids, const uint8_t* const* row_mask, float* const* s, const int64_t* A,
                          const int64_t* off, int64_t D, int64_t B, int64_t C, float* out, int64_t out_ld, void* stream);
int64_t sgnn_readout_many_bwd_workspace_bytes(int64_t n, const int64_t* A, int64_t B, int64_t C);
int sgnn_readout_many_bwd(int64_t n, const float* grad_out, int64_t grad_ld, const float* const* sims, const int64_t* sims_ld,
                          const int64_t* const* sim_col, const float* const* X, const float* const* wp,
                          const float* const* bp, const int64_t* const* ids, const uint8_t* const* row_mask,
                          float* const* s, const int64_t* A, const int64_t* off, int64_t D, int64_t B, int64_t C,
                          float* const* grad_X, float* const* grad_wp, float* const* grad_bp, void* workspace,
                          int64_t workspace_bytes, unsigned* tickets, void* stream);

/* ---------------------------------------------------------------------------------------
 * a18  Embedding-table gradient without atomics (the backward of every op that gathers table rows:
 * autograd of SubGNN/SubGNN.py:609-622, anchor_patch_samplers.py:404-411, subgraph_mpn.py:227-231 as
 * run by loss.backward(), SubGNN/SubGNN.py:1163-1164).
 *   table[key[e], :] += c1[e] * G[row(e), :] + c2[e] * v[:]      for e = order[0], order[1], ...
 * order: the edge numbers sorted STABLY by target key; key_sorted[p] = key of order[p] (ascending); key 0
 * (the PAD row) contributes nothing.  row(e) = edge_row[e], or e / edges_per_row when edge_row is NULL.
 * c1 NULL = 1; c2 / v NULL = no second term; G NULL = only the second term.  arg (nullable, (rows, D) int32):
 * column d of edge e counts only where arg[row(e), d] == key (the max aggregator's argmax).
 * Every table row has one writer and a fixed summation order: results are bit-reproducible.
 * sgnn_mpn_bwd_edges: keys and coefficients of a GATHER message-passing layer's backward (c1 = the edge
 * weight w, c2 = w * grad_z; masked or zero-weight edges get key 0); sgnn_mpn_bwd_wp_partial: that layer's
 * read-out weight gradient as per-row partial sums (R, partial_ld) for the caller to add up; partial_ld = D, or D + 1: then
 * column D holds the row's sum of grad_z (through args->z_act), the per-row partial of the read-out bias's gradient.
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_scatter_add_rows_workspace_bytes(int64_t n_edges, int64_t D);
/* The stable sort the scatter needs: key_sorted / order (int32, n_edges each) from keys in [0, max_key] -- a radix
 * sort over the bits max_key has (rocPRIM), positions as the payload.  An order that does not change between
 * passes (the component members of a split) can be computed once and kept. */
int64_t sgnn_sort_edges_by_key_workspace_bytes(int64_t n_edges, int64_t max_key);
int sgnn_sort_edges_by_key(const int32_t* keys, int64_t n_edges, int64_t max_key, int32_t* key_sorted, int32_t* order,
                           void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_scatter_add_rows_sorted(const int32_t* order, const int32_t* key_sorted, int64_t n_edges,
                                 const int32_t* edge_row, int64_t edges_per_row,
                                 const float* G, int64_t D, const float* c1, const float* c2, const float* v,
                                 const int32_t* arg, float* table,
                                 void* workspace, int64_t workspace_bytes, void* stream);
/* n_lists scatters into ONE table as one sorted list: the edge lists are concatenated (list order, then position), sorted once
 * (stable) and scattered once -- the form a batch-sized training step uses for the 6-18 short lists (1-30 k edges: one per layer
 * body, the component embeddings, the shared anchors' lookups) it adds to the embedding table's gradient: one pack launch, one
 * sort, two scatter launches instead of 6-18 times (sort + two).  keys / n_edges / edge_row / edges_per_row / G / c1 / c2 / v:
 * HOST arrays over the lists, each entry as the argument of that name of sgnn_scatter_add_rows_sorted (DEVICE pointers; every
 * G[k] has D columns; no argmax form).  Every table row has one writer and a fixed order of addition. */
int64_t sgnn_scatter_add_rows_multi_workspace_bytes(int64_t total_edges, int64_t D, int64_t max_key);
int sgnn_scatter_add_rows_multi(int64_t n_lists, const int32_t* const* keys, const int64_t* n_edges,
                                const int32_t* const* edge_row, const int64_t* edges_per_row, const float* const* G,
                                const float* const* c1, const float* const* c2, const float* const* v, int64_t D,
                                int64_t max_key, float* table, void* workspace, int64_t workspace_bytes, void* stream);
/* SHARED source, batch-sized calls, without atomics: per-row-tile partials in the workspace, added in tile order
 * (grad_x (A, D), grad_wp (D) and grad_bp (1) -- the read-out bias's gradient, the sum of every entry of grad_z taken through
 * args->z_act -- are OVERWRITTEN, each may be NULL). */
int64_t sgnn_mpn_bwd_shared_det_workspace_bytes(int64_t R, int64_t A, int64_t D);
int sgnn_mpn_bwd_shared_det(const struct sgnn_mpn_args* args, const float* grad_agg, const float* grad_z,
                            float* grad_x, float* grad_wp, float* grad_bp, void* workspace, int64_t workspace_bytes,
                            void* stream);
int sgnn_mpn_bwd_edges(const struct sgnn_mpn_args* args, const float* grad_z, int32_t* out_keys, float* out_c1,
                       float* out_c2, void* stream);
int sgnn_mpn_bwd_wp_partial(const struct sgnn_mpn_args* args, const float* grad_z, float* partial, int64_t partial_ld,
                            void* stream);
/* sgnn_mpn_bwd_edges for up to sgnn_mpn_fwd_many_max_bodies() GATHER bodies in one launch (HOST arrays of n entries; out_c2[k] /
 * grad_z[k] nullable as in the single form): the edge lists feed the step's combined table-gradient scatter, which runs when the
 * table's gradient is handed over -- until then they can wait for each other. */
int sgnn_mpn_bwd_edges_many(int64_t n, const struct sgnn_mpn_args* args, const float* const* grad_z, int32_t* const* out_keys,
                            float* const* out_c1, float* const* out_c2, void* stream);

/* ---------------------------------------------------------------------------------------
 * a12  update(): out = relu([x | aggr] W^T + b) and its backward (SubGNN/subgraph_mpn.py:233-241 with the
 * nn.Linear(2 D, D) of subgraph_mpn.py:33), one row per component.  x, aggr, out, grad_*: (R, D) float32 row-major;
 * W (D, 2 D); b (D), nullable in the forward.  D in {32, 64, 128} (else SGNN_ERR_UNSUPPORTED_D: the caller keeps
 * the library-GEMM form).  fp32 operands and accumulation (v_mfma_f32_32x32x2_f32).
 * Backward: dpre = grad_out * (out > 0); [grad_x | grad_aggr] = dpre W (either may be NULL: not computed);
 * grad_W = dpre^T [x | aggr], grad_b = column sums of dpre (either may be NULL) -- contracted over row blocks whose
 * partial sums (workspace) are added in block order: bit-reproducible.
 * relu(v) = v <= 0 ? 0 : v: a NaN pre-activation stays NaN as under torch.relu; -Inf and -0 give 0.
 * R == 0: nothing is launched and the pointers of the empty tensors may be NULL (the backward zeroes grad_W / grad_b).
 * A call refused for its arguments (SGNN_ERR_BAD_ARG, SGNN_ERR_UNSUPPORTED_D) has written nothing.
 * ------------------------------------------------------------------------------------- */
int sgnn_update_fwd(const float* x, const float* aggr, const float* W, const float* b, int64_t R, int64_t D,
                    float* out, void* stream);
/* The forward with aggr as the anchor-chunk partial aggregates sgnn_mpn_fwd writes, aggr_chunks (n_chunks, R, D): added in
 * chunk order while they are loaded (no separate reduction launch per layer) and, when aggr_sum (R, D) is given, written out
 * once for sgnn_update_bwd.  n_chunks > 1 needs R <= sgnn_update_fwd_chunks_max_rows() (the batch-sized launch shape: the
 * only one sgnn_mpn_fwd splits). */
int64_t sgnn_update_fwd_chunks_max_rows(void);
int sgnn_update_fwd_chunks(const float* x, const float* aggr_chunks, int64_t n_chunks, const float* W, const float* b,
                           int64_t R, int64_t D, float* out, float* aggr_sum, void* stream);
/* The update layers of n bodies of ONE message-passing layer (up to sgnn_update_many_max_bodies() channel sides of a batch-sized
 * step: same R <= sgnn_update_fwd_chunks_max_rows(), same D) in one launch each way -- forward 1 launch, backward 3 (dx, dW
 * partials, reduce) instead of n and 3 n.  All pointer tables are HOST arrays of n DEVICE pointers with the meaning of the
 * single-body arguments; aggr_chunks[k] is (n_chunks[k], R, D), its sum goes to aggr_sum[k] (required when n_chunks[k] > 1).
 * Backward: grad_out[k] NULL = body k received no gradient and is skipped; else grad_x[k] / grad_aggr[k] may be NULL and
 * grad_W[k], grad_b[k] are both written; workspace n * sgnn_update_bwd_workspace_bytes(R, D). */
int64_t sgnn_update_many_max_bodies(void);
int sgnn_update_fwd_many(int64_t n, const float* const* x, const float* const* aggr_chunks, const int64_t* n_chunks,
                         const float* const* W, const float* const* b, int64_t R, int64_t D, float* const* out,
                         float* const* aggr_sum, void* stream);
int sgnn_update_bwd_many(int64_t n, const float* const* grad_out, const float* const* out, const float* const* x,
                         const float* const* aggr, const float* const* W, int64_t R, int64_t D, float* const* grad_x,
                         float* const* grad_aggr, float* const* grad_W, float* const* grad_b, void* workspace,
                         int64_t workspace_bytes, void* stream);
int64_t sgnn_update_bwd_workspace_bytes(int64_t R, int64_t D);
int sgnn_update_bwd(const float* grad_out, const float* out, const float* x, const float* aggr, const float* W,
                    int64_t R, int64_t D, float* grad_x, float* grad_aggr, float* grad_W, float* grad_b,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * a18  Adam on one float32 buffer of any length n in one pass (torch.optim.Adam's rule, no amsgrad: SubGNN/SubGNN.py:1156-1161),
 * with the gradient term in one of two forms:
 *   weight_decay == 0: g * grad_scale -- grad_scale (nullable: 1) is the caller's clip coefficient (train_config.py:
 *     gradient_clip_val) as a DEVICE scalar, so the clip needs no host round trip (dist.ShardedTableAdam's owned slice);
 *   weight_decay != 0: g + weight_decay * param -- torch.optim.Adam(lr, weight_decay)'s coupled L2 (the node-embedding
 *     trainer: prepare_dataset/train_node_emb.py:99); grad_scale must then be null.
 * step = 1 for the first update.  All four arrays float32[n], 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
int sgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, void* stream);

/* a18c  The whole optimizer tail of a step -- clip_grad_norm_ over ALL parameters (train_config.py: Trainer(gradient_clip_val))
 * followed by torch.optim.Adam over all of them (SubGNN/SubGNN.py:1156-1161) -- in two launches per 72 tensors.  The tensor lists
 * are HOST arrays of DEVICE pointers (float32, 4-byte aligned at least; 16-byte aligned tensors take the vector path), numels[i]
 * elements each.
 *   sgnn_optim_partials(numels, n)          how many floats sgnn_optim_sumsq writes (one per workgroup; -1 = bad argument)
 *   sgnn_optim_sumsq(grads, ...)            per-workgroup sums of squares of every gradient -> partial[]; the step counts
 *                                           step_counters[counter_slots[i]] (step_counters nullable: DEVICE int64[]; counter_slots
 *                                           nullable: HOST int64[n_tensors], default i) each advance by one in the same launch
 *   sgnn_optim_count(step_counters, ...)    the advance alone (a step without clipping)
 *   sgnn_optim_adam(...)                    every workgroup adds partial[0..n_partial) in one fixed order, forms
 *                                           coefficient = min(1, max_norm / (sqrt(sum) + 1e-6)) and updates its chunk with the
 *                                           gradient times the coefficient (max_norm <= 0: no clipping, partial unused).
 *                                           Step counts: EXACTLY ONE of steps (HOST int64[n_tensors], >= 1: this update's
 *                                           number, per tensor) and step_counters (DEVICE, tensor i reads step_counters[counter_slots[i]] after
 *                                           sgnn_optim_sumsq / sgnn_optim_count advanced them -- the form a recorded step replays).
 *                                           zero_grad (nullable HOST int32[n_tensors]): != 0 zeroes that gradient in the same
 *                                           pass.  coef_out (nullable DEVICE float[2]): the coefficient and the total norm.
 *                                           row_lens / row_seen (both nullable HOST arrays): tensor i is a table of rows of
 *                                           row_lens[i] floats (a power of two, 4..256) with one DEVICE byte per row,
 *                                           row_seen[i] (zero-initialised by the caller, owned by the optimizer state): set once
 *                                           the row has had a non-zero gradient.  A row with an all-zero gradient and a clear
 *                                           byte has m = v = 0 and Adam's update of it is exactly zero: it is skipped after the
 *                                           read of its gradient (one such table per launch; bit-identical to the dense update).
 * The gradients themselves are NOT scaled in memory (clip_grad_norm_ scales them in place; here they are consumed). */
int64_t sgnn_optim_partials(const int64_t* numels, int64_t n_tensors);
int sgnn_optim_sumsq(const float* const* grads, const int64_t* numels, int64_t n_tensors, float* partial,
                     int64_t* step_counters, const int64_t* counter_slots, void* stream);
int sgnn_optim_count(int64_t* step_counters, const int64_t* counter_slots, int64_t n_tensors, void* stream);
int sgnn_optim_adam(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, float lr, float beta1, float beta2,
                    float eps, const int64_t* steps, const int64_t* step_counters, const int64_t* counter_slots,
                    const int64_t* row_lens, unsigned char* const* row_seen,
                    const float* partial, int64_t n_partial, float max_norm, float* coef_out, void* stream);
/*   sgnn_optim_adam_lr_table(...)           sgnn_optim_adam with the learning rate read on the device: lr_table (DEVICE float[lr_len],
 *                                           lr_len >= 1) in place of lr.  The update of step s (the step count the tensor reads
 *                                           above) takes lr_table[min(s, lr_len) - 1]: a range test's schedule replays from one
 *                                           recording; lr_len = 1 is a constant rate on the device.  Same arithmetic as the host
 *                                           float: a table holding lr gives sgnn_optim_adam's result bit for bit. */
int sgnn_optim_adam_lr_table(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                             const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, const float* lr_table,
                             int64_t lr_len, float beta1, float beta2, float eps, const int64_t* steps,
                             const int64_t* step_counters, const int64_t* counter_slots, const int64_t* row_lens,
                             unsigned char* const* row_seen, const float* partial, int64_t n_partial, float max_norm,
                             float* coef_out, void* stream);
/*   sgnn_optim_adam_ema(...)                sgnn_optim_adam that also moves a weight average: ema (HOST array of DEVICE
 *   sgnn_optim_adam_ema_lr_table(...)       pointers, one float32 tensor per parameter, 4-byte aligned at least) after the
 *                                           update of every element it steps: e = fma(w, p_new - e, e), w = 1 - d_s (formed once
 *                                           per workgroup, in double), d_s = ema_decay (in [0, 1)), or with ema_warmup != 0
 *                                           min(ema_decay, (1 + s) / (10 + s)) at the step count s the tensor reads above.
 *                                           Parameters, moments and the coefficient are sgnn_optim_adam's bit for bit.  The
 *                                           average advances with the tensor's OWN steps: a tensor outside the call keeps its
 *                                           average, and so does a table row the update skips -- with the average initialised to
 *                                           the parameter such a row has e == p bit for bit, which e + w (p - e) leaves as it
 *                                           is, so skipping needs no catch-up.  A NaN coefficient steps every row and the
 *                                           averages turn NaN with the parameters.  56 tensors per launch (the fifth pointer).
 *   sgnn_optim_swap(a, b, numels, n, ...)   a[i] <-> b[i] in place (HOST arrays of DEVICE pointers, numels[i] floats, 4-byte
 *                                           aligned at least; float4 where both are 16-byte aligned), no temporary, one launch
 *                                           per 128 tensors; empty tensors and a[i] == b[i] are skipped, a partial overlap is
 *                                           a bad argument. */
int sgnn_optim_adam_ema(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, float lr, float beta1, float beta2,
                        float eps, const int64_t* steps, const int64_t* step_counters, const int64_t* counter_slots,
                        const int64_t* row_lens, unsigned char* const* row_seen, const float* partial, int64_t n_partial,
                        float max_norm, float* coef_out, float* const* ema, float ema_decay, int ema_warmup, void* stream);
int sgnn_optim_adam_ema_lr_table(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                 const int64_t* numels, const int32_t* zero_grad, int64_t n_tensors, const float* lr_table,
                                 int64_t lr_len, float beta1, float beta2, float eps, const int64_t* steps,
                                 const int64_t* step_counters, const int64_t* counter_slots, const int64_t* row_lens,
                                 unsigned char* const* row_seen, const float* partial, int64_t n_partial, float max_norm,
                                 float* coef_out, float* const* ema, float ema_decay, int ema_warmup, void* stream);
int sgnn_optim_swap(float* const* a, float* const* b, const int64_t* numels, int64_t n_tensors, void* stream);


/* A batch's rows of up to sgnn_gather_rows_many_max() per-split tensors in ONE launch (the row gathers of _pad_collate,
 * SubGNN/SubGNN.py:1068-1114: component ids, border ids, the channels' similarity rows, labels): dst[t][i, :] =
 * src[t][idx[i], :] with rows as raw bytes -- row_bytes[t] each, src_rows[t] rows in the source.  An index outside the source
 * (index_select raises for it) yields a ZERO row and sets *out_of_range (nullable DEVICE int32, never cleared here) to 1: the
 * caller polls the flag.  n * B up to 2^30 (the pair travels in blockIdx.x).
 * src / dst / row_bytes / src_rows: HOST arrays (src / dst of DEVICE pointers); idx: DEVICE int64[B]. */
int64_t sgnn_gather_rows_many_max(void);
int sgnn_gather_rows_many(int64_t n, const void* const* src, void* const* dst, const int64_t* row_bytes,
                          const int64_t* src_rows, const int64_t* idx, int64_t B, int32_t* out_of_range, void* stream);

/* ---------------------------------------------------------------------------------------
 * a16/a17 fused  The MLP head of SubGNN.forward + the loss of a training step (SubGNN/SubGNN.py:304-312: lin -> relu -> dropout
 * -> lin2 -> relu -> dropout -> lin3; SubGNN.py:1116-1124: nn.CrossEntropyLoss + subgraph_utils.calc_accuracy) behind the first
 * layer's GEMM: z1 = x W1^T + b1 (B, H1) comes from the caller's library GEMM, as does dx = dz1 W1 in the backward.
 *   sgnn_head_supported(H1, H2, K)   1 when the widths fit the kernels' LDS tables (H1, H2 <= 128, K <= 32)
 *   sgnn_head_blocks(B)              workgroups of either launch; the backward writes sgnn_head_partial_floats(H1, H2, K) floats
 *                                    per workgroup: [gW3 (K H2) | gb3 (K) | gW2 (H2 H1) | gb2 (H2) | gb1 (H1)], to be added over the
 *                                    workgroups in order (sgnn_reduce_partials)
 *   sgnn_head_fwd    a1 = drop(relu(z1)) (B, H1), a2 = drop(relu(a1 W2^T + b2)) (B, H2), logits = a2 W3^T + b3 (B, K); with labels
 *                    (int64 in [0, K) or -100, nullable) also lse (B + 1 floats, [B] = rows counted) and out = [mean loss,
 *                    accuracy over all B rows, rows counted].  p: dropout probability of both layers; p > 0 reads rng =
 *                    DEVICE int64[2] {seed, step} and ADVANCES step by one (the last workgroup does, after every workgroup has read
 *                    it): masks are a pure function of (seed, step, layer, element), so a step replayed from a hipGraph draws new
 *                    ones.  workspace: sgnn_head_fwd_workspace_bytes(B) bytes, its last 16 bytes ZERO before the first call (a
 *                    ticket the launch leaves zero).  Loss partials are added in workgroup order: bit-reproducible.
 *   sgnn_head_bwd    dlogits = (softmax - onehot) grad_loss[0] / rows[0] (+ grad_logits, nullable) -> dz1 (B, H1) and the
 *                    per-workgroup partials above.  grad_loss nullable (then only grad_logits flows).
 * ------------------------------------------------------------------------------------- */
int sgnn_head_supported(int64_t H1, int64_t H2, int64_t K);
int64_t sgnn_head_blocks(int64_t B);
int64_t sgnn_head_partial_floats(int64_t H1, int64_t H2, int64_t K);
int64_t sgnn_head_fwd_workspace_bytes(int64_t B);
int sgnn_head_fwd(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                  const float* W3, const float* b3, const int64_t* labels, float p, int64_t* rng, float* a1, float* a2,
                  float* logits, float* lse, float* out, void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_head_bwd(const float* logits, const float* lse, const int64_t* labels, const float* grad_loss,
                  const float* grad_logits, const float* rows, const float* a1, const float* a2, const float* W2,
                  const float* W3, int64_t B, int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial,
                  void* stream);

/* The same head in multi-label mode (nn.BCEWithLogitsLoss, SubGNN/SubGNN.py:133; exact-match accuracy, SubGNN/subgraph_utils.py:
 * 108-124): kernels of their own, so the single-label launches above carry nothing for it.  targets: (B, K) int64 indicator
 * matrix (non-zero counts as 1, not nullable).  out = [sum of the element losses / (B K), rows whose K predictions
 * (1 / (1 + exp(-x)) > 0.5 in float32) all equal their targets / B, B K].  No lse: the backward recomputes
 * dlogits = (sigmoid(x) - y) grad_loss[0] / rows[0] (+ grad_logits, nullable) from the logits; rows = out + 2.  Workspace, ticket,
 * partials, summation order, dropout masks and the {seed, step} state are those of sgnn_head_fwd / sgnn_head_bwd. */
int sgnn_head_fwd_ml(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                     const float* W3, const float* b3, const int64_t* targets, float p, int64_t* rng, float* a1, float* a2,
                     float* logits, float* out, void* workspace, int64_t workspace_bytes, void* stream);
int sgnn_head_bwd_ml(const float* logits, const int64_t* targets, const float* grad_loss, const float* grad_logits,
                     const float* rows, const float* a1, const float* a2, const float* W2, const float* W3, int64_t B,
                     int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial, void* stream);

/* The head's four launches with class weights (torch's `weight` of nn.CrossEntropyLoss, `weight` / `pos_weight` of
 * nn.BCEWithLogitsLoss: the loss modules built at SubGNN/SubGNN.py:133; semantics as stated at sgnn_cross_entropy_fwd_weighted).
 * The argument lists are those of the four entries above plus the weight rows at the end: DEVICE pointers to K <= 32 floats,
 * nullable; with every row null -- or without labels / grad_loss -- the call IS the bare entry, and the bare entries forward here
 * with nulls.  Otherwise kernels of their own run (the bare kernels carry no argument and no branch for weights): the rows are
 * loaded into LDS once per workgroup.  Single-label: out[2] = lse[B] = the sum of the counted rows' weights, which is what
 * sgnn_head_bwd_weighted divides by through `rows`; class weights of 1.0 give the bare result bit for bit.  Multi-label: out[2] = B K
 * as before.  Accuracy, logits, saved activations, dropout masks and the {seed, step} state do not depend on the weights. */
int sgnn_head_fwd_weighted(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                           const float* W3, const float* b3, const int64_t* labels, float p, int64_t* rng, float* a1, float* a2,
                           float* logits, float* lse, float* out, void* workspace, int64_t workspace_bytes, void* stream,
                           const float* class_weight);
int sgnn_head_bwd_weighted(const float* logits, const float* lse, const int64_t* labels, const float* grad_loss,
                           const float* grad_logits, const float* rows, const float* a1, const float* a2, const float* W2,
                           const float* W3, int64_t B, int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial,
                           void* stream, const float* class_weight);
int sgnn_head_fwd_ml_weighted(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                              const float* W3, const float* b3, const int64_t* targets, float p, int64_t* rng, float* a1,
                              float* a2, float* logits, float* out, void* workspace, int64_t workspace_bytes, void* stream,
                              const float* weight, const float* pos_weight);
int sgnn_head_bwd_ml_weighted(const float* logits, const int64_t* targets, const float* grad_loss, const float* grad_logits,
                              const float* rows, const float* a1, const float* a2, const float* W2, const float* W3, int64_t B,
                              int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial, void* stream,
                              const float* weight, const float* pos_weight);

/* The head's four launches with a shaped loss (label smoothing / focal loss; semantics as stated at
 * sgnn_cross_entropy_fwd_shaped).  The argument lists are those of the four _weighted entries plus `float label_smoothing, float
 * focal_gamma` (the _ml entries: focal_gamma only).  With both 0 -- or without labels / grad_loss -- the call IS the _weighted entry;
 * a value outside its domain or both non-zero: SGNN_ERR_BAD_ARG before any launch.  Otherwise kernels of their own run, with the
 * weight rows in LDS (an absent row stands as ones) and {label_smoothing, focal_gamma} passed by value, so a recorded step replays
 * them.  The backward recomputes what it needs from logits and lse: nothing more is saved.  out[2] = lse[B] stays the divisor;
 * accuracy, logits, saved activations, dropout masks and the {seed, step} state do not depend on the loss mode. */
int sgnn_head_fwd_shaped(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                         const float* W3, const float* b3, const int64_t* labels, float p, int64_t* rng, float* a1, float* a2,
                         float* logits, float* lse, float* out, void* workspace, int64_t workspace_bytes, void* stream,
                         const float* class_weight, float label_smoothing, float focal_gamma);
int sgnn_head_bwd_shaped(const float* logits, const float* lse, const int64_t* labels, const float* grad_loss,
                         const float* grad_logits, const float* rows, const float* a1, const float* a2, const float* W2,
                         const float* W3, int64_t B, int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial,
                         void* stream, const float* class_weight, float label_smoothing, float focal_gamma);
int sgnn_head_fwd_ml_shaped(const float* z1, int64_t B, int64_t H1, int64_t H2, int64_t K, const float* W2, const float* b2,
                            const float* W3, const float* b3, const int64_t* targets, float p, int64_t* rng, float* a1,
                            float* a2, float* logits, float* out, void* workspace, int64_t workspace_bytes, void* stream,
                            const float* weight, const float* pos_weight, float focal_gamma);
int sgnn_head_bwd_ml_shaped(const float* logits, const int64_t* targets, const float* grad_loss, const float* grad_logits,
                            const float* rows, const float* a1, const float* a2, const float* W2, const float* W3, int64_t B,
                            int64_t H1, int64_t H2, int64_t K, float p, float* dz1, float* partial, void* stream,
                            const float* weight, const float* pos_weight, float focal_gamma);

/* A^T B for tall operands (the weight gradients of Linear / LSTM layers: outputs of a few thousand elements contracted over
 * thousands of rows -- a library GEMM runs them on a handful of workgroups): job k contracts A[k] (R[k], M[k]) with B[k]
 * (R[k], N[k]), row strides lda / ldb floats, over blocks of rows on the matrix cores (fp32 MFMA, fp32 accumulate) and writes
 * part[k] = (sgnn_contract_rows_blocks(R[k], M[k], N[k]), M[k], N[k]) block partials; sgnn_reduce_partials adds them in block order (a fixed
 * order: bit-reproducible).  colsum_part (nullable; entries nullable): job k also writes (blocks, M[k]) partial COLUMN SUMS of A[k]
 * (a bias gradient rides along with its weight's).  Up to sgnn_contract_rows_max_jobs() jobs per launch.  All arrays are HOST arrays (of DEVICE
 * pointers where they hold pointers).
 * sgnn_reduce_partials: out[k][j] = sum_b part[k][b * n[k] + j] over n_blocks[k] blocks, up to sgnn_reduce_partials_max_jobs()
 * jobs per launch. */
int64_t sgnn_contract_rows_max_jobs(void);
int64_t sgnn_contract_rows_blocks(int64_t R, int64_t M, int64_t N);
int sgnn_contract_rows_partial(int64_t n_jobs, const float* const* A, const float* const* B, const int64_t* lda,
                               const int64_t* ldb, const int64_t* M, const int64_t* N, const int64_t* R,
                               float* const* part, float* const* colsum_part, void* stream);
int64_t sgnn_reduce_partials_max_jobs(void);
int sgnn_reduce_partials(int64_t n_jobs, const float* const* part, const int64_t* n_blocks, const int64_t* n,
                         float* const* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * a19  Node-embedding pre-training (reference prepare_dataset/train_node_emb.py:40-110, model.py:15-36, utils.py:22-56,
 * preprocess.py:38-60): two graph convolutions over one-hot features -- so layer 1 aggregates a trainable (N, hidden) table --
 * and link prediction on dot products, full-batch over the whole graph.  All fp32, deterministic, no float atomics.
 *
 * sgnn_ne_aggregate replaces PyG's GINConv / GCNConv propagate (model.py:20-27; PyG gcn_norm for the GCN weights):
 *   out[v] = a_self[v] X[v] + sum_{e = rowptr[v] .. rowptr[v+1]} w[e] X[col[e]] (+ bias), v < n_rows, X and out (n_rows, F),
 * then relu != 0: max(., 0), then drop_thr != 0: element (v, f) kept iff (draw64(seed, stream_id, v, f) >> 32) >= drop_thr and
 * scaled by drop_scale, else 0 (model.py:33-34, F.dropout).  a_self / w / bias nullable (1, 1, none).  F a multiple of 4, at most
 * 512 (else SGNN_ERR_UNSUPPORTED_D).  Rows longer than sgnn_ne_chunk_entries() entries are summed by chunks: the caller lists them
 * as chunk items (chunk_row[c], first entry chunk_beg[c]; a row's chunks consecutive and in entry order) and as long rows
 * (long_rows[r], chunks chunk_first[r] .. chunk_first[r+1]); partial holds n_chunks x F floats.  The backward (dX = A^T dOut) is
 * the same call over the transposed CSR.
 * sgnn_ne_relu_drop_bwd: dst = out > 0 ? grad * scale : 0 (dst may be grad) -- the gradient through relu -> dropout from the OUTPUT of
 * that epilogue (an element passed both iff it is positive); n a multiple of 4.
 * sgnn_ne_negatives replaces torch_geometric.utils.negative_sampling (train_node_emb.py:60,69): pair i takes the first attempt
 * a < max_attempts of d = draw64(seed, stream_id, item_base + i, a), u = 1 + ((d >> 32) n_ids >> 32), v = 1 + ((d mod 2^32)
 * n_ids >> 32) with u != v and v not in u's ascending adjacency row col_sorted[rowptr[u] .. rowptr[u+1]); (0, 0) when none is.
 * sgnn_ne_link_loss replaces utils.el_dot + calc_loss_both (utils.py:22-56): for pairs p < n_pairs (label 1 for p < n_pos, else 0)
 * s = sigmoid(Z[pu[p]] . Z[pv[p]]) -> s_out, d loss / d dot -> g_out (nullable), loss = mean of
 * nll(log_softmax(stack(1 - s, s)), y) -> loss[0], reduced in a fixed order; workspace sgnn_ne_link_loss_workspace_bytes().
 * The optimiser, torch.optim.Adam(lr, weight_decay) (train_node_emb.py:99), is sgnn_adam_step with weight_decay (a18).
 * ------------------------------------------------------------------------------------- */
int64_t sgnn_ne_chunk_entries(void);
int sgnn_ne_aggregate(const int64_t* rowptr, const int32_t* col, const float* w, const float* a_self, const float* X,
                      const float* bias, int64_t n_rows, int64_t F, const int32_t* chunk_row, const int64_t* chunk_beg,
                      int64_t n_chunks, const int32_t* long_rows, const int64_t* chunk_first, int64_t n_long,
                      int relu, uint32_t drop_thr, float drop_scale, uint64_t seed, uint64_t stream_id, float* out,
                      float* partial, void* stream);
int sgnn_ne_relu_drop_bwd(const float* grad, const float* out, float* dst, int64_t n, float scale, void* stream);
int sgnn_ne_negatives(const int64_t* rowptr, const int32_t* col_sorted, int64_t n_ids, int64_t n, uint64_t seed,
                      uint64_t stream_id, int64_t item_base, int max_attempts, int32_t* u_out, int32_t* v_out, void* stream);
int64_t sgnn_ne_link_loss_workspace_bytes(void);
int sgnn_ne_link_loss(const float* Z, int64_t F, const int32_t* pu, const int32_t* pv, int64_t n_pairs, int64_t n_pos,
                      float* s_out, float* g_out, float* loss, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): streaming copy of n_bytes with 4 or 16 bytes per lane.
 * The rocprofv3 memory-side counters (FETCH_SIZE / WRITE_SIZE) are calibrated on it -- a known byte
 * count in the access width of the CSR gather -- before they are read as HBM traffic of
 * sgnn_degree_sequence (tools/degseq_hbm_probe.py, bench.py roofline.traffic).
 * ------------------------------------------------------------------------------------- */
int sgnn_probe_stream_copy(const void* src, void* dst, int64_t n_bytes, int bytes_per_lane, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGNN_HIP_H */
