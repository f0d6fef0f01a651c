// The two structures every workgroup kernel over ragged node sets keeps per set (graph_sets.hip, degree_sequence.hip,
// subgraph_props.hip): an open-addressing table node id -> membership or first position, and a lock-free union-find.
//
// Tiers, by the number of ENTRIES of a set: up to SGNN_SET_WAVE_MAX one wavefront holds the set in its lanes (those kernels
// have structures of their own); up to SGNN_SET_LDS_MAX the table lives in LDS (SGNN_SET_LDS_HASH slots: load <= 1/2); beyond
// that in the caller's workspace, every set in a region of its own at the set's offset (4 slots per entry, of which the
// smallest power of two >= 2 n is used: load in (1/4, 1/2]).
//
// The home is a template argument (bool LDS) because it decides how the table may be READ.  Inserts are atomics -- on LDS, or
// on the L2 for the workspace -- and the other stores are plain.  In LDS a plain load behind __threadfence_block() +
// __syncthreads() sees them.  In the workspace it need not: a plain load may be served from a line of the CU's vector L1 that
// was fetched before the insert.  A barrier of the own workgroup does not rule that out, because the regions are not
// line-aligned (a region starts at byte 16 beg; with 2049 entries the 128-byte line of its last used slot also holds the
// first slots of the next set's region), so another workgroup on the same CU, at work on the neighbouring set, can pull the
// shared line in at any time.  Hence idt_ld<false> is a relaxed agent-scope atomic load, which is served by the L2, and
// idt_sync<false> fences device-wide.  Results never depend on the home or on the slot rule.
#pragma once
#include "common.h"

#define SGNN_SET_WAVE_MAX 64                                // up to here one wavefront per set
#define SGNN_SET_LDS_MAX 2048                               // == ops.CC_LDS_MAX: beyond it the tables are in the workspace
#define SGNN_SET_LDS_HASH_BITS 12
#define SGNN_SET_LDS_HASH (1 << SGNN_SET_LDS_HASH_BITS)     // slots of a table in LDS

template <bool LDS> __device__ __forceinline__ int32_t idt_ld(const int32_t* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what the workgroup wrote to its tables before is visible to all of it behind this
template <bool LDS> __device__ __forceinline__ void idt_sync() {
    if (LDS) __threadfence_block(); else __threadfence();
    __syncthreads();
}

// key: 0 = empty slot (ids are >= 1).  pos (optional): the smallest position at which the slot's id was inserted.
// 2^(32 - shift) slots; the slot of an id is the top bits of its hash.
struct IdTable { int32_t* key; int32_t* pos; int shift; };

__device__ __forceinline__ uint32_t idt_slots(const IdTable& t) { return 1u << (32 - t.shift); }
__device__ __forceinline__ uint32_t idt_slot(const IdTable& t, int32_t v) { return sgnn_hash32((uint32_t)v) >> t.shift; }

__device__ __forceinline__ IdTable idt_in_lds(int32_t* key, int32_t* pos = nullptr) {      // SGNN_SET_LDS_HASH slots each
    return IdTable{key, pos, 32 - SGNN_SET_LDS_HASH_BITS};
}

// The region of the set of n > 1 entries at offset beg (< 2^28) of a workspace: keys at ws + 4 beg; positions, where the caller
// has them, at the same offset of their own 4-slots-per-entry array.
__device__ __forceinline__ IdTable idt_in_workspace(int32_t* ws, int64_t beg, int n, int32_t* pos_base = nullptr) {
    return IdTable{ws + 4 * beg, pos_base ? pos_base + 4 * beg : nullptr, __clz(2 * n - 1)};
}

template <bool POS> __device__ __forceinline__ void idt_clear(const IdTable& t, int tid, int threads) {
    for (uint32_t i = tid; i < idt_slots(t); i += threads) { t.key[i] = 0; if (POS) t.pos[i] = 0x7fffffff; }
}

// id v (>= 1) of position i; an id inserted more than once holds one slot (POS: and its smallest position)
template <bool POS> __device__ __forceinline__ void idt_insert(const IdTable& t, int32_t v, int i = 0) {
    const uint32_t mask = idt_slots(t) - 1;
    uint32_t h = idt_slot(t, v);
    while (true) {
        const int32_t old = atomicCAS(&t.key[h], 0, v);
        if (old == 0 || old == v) break;
        h = (h + 1) & mask;
    }
    if (POS) atomicMin(&t.pos[h], i);
}

// slot of id v, -1 = not in the table
template <bool LDS> __device__ __forceinline__ int idt_probe(const IdTable& t, int32_t v) {
    const uint32_t mask = idt_slots(t) - 1;
    uint32_t h = idt_slot(t, v);
    while (true) {
        const int32_t k = idt_ld<LDS>(t.key + h);
        if (k == v) return (int)h;
        if (k == 0) return -1;
        h = (h + 1) & mask;
    }
}

template <bool LDS> __device__ __forceinline__ bool idt_contains(const IdTable& t, int32_t v) { return idt_probe<LDS>(t, v) >= 0; }

template <bool LDS> __device__ __forceinline__ int idt_first(const IdTable& t, int32_t v) {     // first position of id v, -1 = absent
    const int h = idt_probe<LDS>(t, v);
    return h < 0 ? -1 : idt_ld<LDS>(t.pos + h);
}

// the whole workgroup: the table of nodes[0, n), readable when it returns
template <bool LDS, bool POS>
__device__ __forceinline__ void idt_build(const IdTable& t, const int32_t* __restrict__ nodes, int n, int tid, int threads) {
    idt_clear<POS>(t, tid, threads);
    idt_sync<LDS>();
    for (int i = tid; i < n; i += threads) idt_insert<POS>(t, nodes[i], i);
    idt_sync<LDS>();
}

// ---- union-find over the positions of a set: the larger root is hooked under the smaller, so that a component's root is its
// smallest position.  Lock-free; parents are read by the table's rule.
template <bool LDS> __device__ __forceinline__ int uf_find(const int32_t* par, int x) {
    int p = idt_ld<LDS>(par + x);
    while (p != x) { x = p; p = idt_ld<LDS>(par + x); }
    return x;
}

template <bool LDS> __device__ __forceinline__ bool uf_union(int32_t* par, int x, int y) {      // true: this call hooked a root
    while (true) {
        x = uf_find<LDS>(par, x);
        y = uf_find<LDS>(par, y);
        if (x == y) return false;
        if (x < y) { const int t = x; x = y; y = t; }
        if (atomicCAS(&par[x], x, y) == x) return true;
    }
}
