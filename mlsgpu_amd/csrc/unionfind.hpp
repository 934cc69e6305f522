/*
 * Lock-free union-find on the device, shared by the mesh sink's components (mesher.hip), the topology report
 * (topology.hip) and the hole filling (fill.hip): parent[] starts as the identity, unite() hooks the larger root under the smaller with a CAS, and a
 * finished component's root is its smallest id whatever the schedule.
 */
#ifndef MLSGPU_AMD_UNIONFIND_HPP
#define MLSGPU_AMD_UNIONFIND_HPP

#include "common.hpp"

namespace mlsgpu
{

#ifdef __HIPCC__

/* parent[] is read while other workgroups hook roots: the loads must come from the coherence point (a line cached
 * in this CU's vector L1 would never show the new parent and the retry loop below would not end) */
__device__ __forceinline__ uint32_t loadParent(const uint32_t *parent, uint32_t v)
{
    return __hip_atomic_load(&parent[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t findRoot(const uint32_t *parent, uint32_t v)
{
    uint32_t p = loadParent(parent, v);
    while (p != v)
    {
        v = p;
        p = loadParent(parent, v);
    }
    return v;
}

/* findRoot that shortens LONG walks: a start vertex more than `shortcut` steps from its root is re-parented to the root.
 * Parents only ever point to SMALLER ids and hooks re-parent roots only, so an ancestor stays an ancestor whatever the other
 * workgroups do meanwhile: a stale or lost store costs time, never correctness, and the root of a finished component is its
 * smallest id either way (the result does not depend on the schedule).  Measured: unconditional pointer jumping (a store
 * per step) takes the shells cloud's finalize from 17.4 to 14.3 ms but the noise cloud's from 96.5 to 115.9 (its chains are
 * short already: the stores are pure cost there); the shortcut beyond 1 / 3 / 8 steps: shells 13.3 / 12.8 / 14.1 ms, noise
 * 113.9 / 103.9 / 96.3 against 17.9 and 97.4 without.
 * Round 4: the threshold is a launch parameter chosen by the size of the mesh (unionShortcut in mesher.hip): surface-like jobs
 * (tens of millions of vertices in a handful of sheets: long chains) take 3, the hundreds of millions of vertices of a noise
 * cloud 8. */
__device__ __forceinline__ uint32_t findRootHalving(uint32_t *parent, uint32_t v, uint32_t shortcut)
{
    const uint32_t start = v;
    uint32_t steps = 0;
    uint32_t p = loadParent(parent, v);
    while (p != v)
    {
        v = p;
        p = loadParent(parent, v);
        steps++;
    }
    if (steps > shortcut)
        __hip_atomic_store(&parent[start], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}

/* the `shortcut` of a mesh that is a surface: what the stages that work on one chunk pass (topology.hip, fill.hip) */
const uint32_t UNION_SHORTCUT = 3;

/* the sets of a and b become one; *failed is set (and the call gives up) if the retry bound is ever reached */
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t *failed, uint32_t shortcut)
{
    for (uint32_t attempt = 0;; attempt++)
    {
        if (attempt == (1u << 20))      /* cannot happen; a bound instead of a hung GPU if it ever does */
        {
            *failed = 1;
            break;
        }
        a = findRootHalving(parent, a, shortcut);
        b = findRootHalving(parent, b, shortcut);
        if (a == b)
            break;
        if (a < b)
        {
            const uint32_t s = a; a = b; b = s;
        }
        /* hook the larger root under the smaller; retry if someone re-parented it first */
        if (atomicCAS(&parent[a], a, b) == a)
            break;
    }
}

#endif /* __HIPCC__ */

} // namespace mlsgpu

#endif
