// gs_unionfind.h -- find and unite over a u32 parent array, for the component labelling of gs_components.hip.  Also plain
// C++: a host program that defines none of the macros below replays the kernels' phases sequentially with the same code
// (tests/cpp/components_merge.cpp).
//
// The array holds a forest: parent[i] == i marks a root, and parent[i] <= i ALWAYS, so that a chain of parents is strictly
// decreasing until it reaches its root: find() ends after at most i steps whatever other threads do meanwhile, because the
// only writes ever made lower an entry (unite: an atomic minimum with a smaller index; the flatten phase: the root found,
// which is not larger than the entry it replaces).  Nothing here waits for another thread.
#pragma once
#include <stdint.h>

#ifndef GS_UF_FN
#define GS_UF_FN inline // (the kernels: __device__ __forceinline__)
#endif
#ifndef GS_UF_LOAD
#define GS_UF_LOAD(p) (*(p)) // (the kernels: a relaxed atomic load -- another thread may lower the entry at any time)
#endif
#ifndef GS_UF_MIN
// The old value of *p, which becomes min(*p, v).  (The kernels: atomicMin.)
static inline uint32_t gs_uf_host_min(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
}
#define GS_UF_MIN(p, v) gs_uf_host_min((p), (v))
#endif

constexpr uint32_t kUfUnset = 0xffffffffu; // the entry of a cell that is not set: never followed, never united

// The root of x's tree: strictly decreasing indices, no writes.
GS_UF_FN uint32_t gs_uf_find(uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = GS_UF_LOAD(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// Makes the trees of a and b one.  The larger of the two roots is hung under the smaller with an atomic minimum; if the
// larger was no root any more -- another thread had hung it under `old` meanwhile, old < a -- the entry is now
// min(old, b) and still leads to one of the two, and the union that remains to be made is that of old and b: a retry
// always starts from a smaller index than the one before, so the loop ends.
GS_UF_FN void gs_uf_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = gs_uf_find(parent, a);
        b = gs_uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = GS_UF_MIN(parent + a, b);
        if (old == a) return;
        a = old;
    }
}
