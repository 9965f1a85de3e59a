// The lock-free union-find of csrc/components.hip and csrc/branches.hip: a forest in an int32 array L where L[i] is the PARENT of i, with
// parent(i) <= i and equality exactly for a root.  The discipline (coherence, termination) is written out at the top of components.hip:
// L is read only with relaxed atomic loads of scope SCOPE or through the value an atomic min returned, and written only with that atomic;
// a slot only ever decreases; every loop strictly decreases the index it holds; nothing waits for another lane or workgroup.
#pragma once
#include <hip/hip_runtime.h>

#define CC_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT

template <int SCOPE>
__device__ __forceinline__ int cc_load(const int* L, int i) {
  return __hip_atomic_load(L + i, __ATOMIC_RELAXED, SCOPE);
}

// the root of i as far as the loads show it; i strictly decreases
template <int SCOPE>
__device__ __forceinline__ int cc_find(const int* L, int i) {
  for (;;) {
    const int p = cc_load<SCOPE>(L, i);
    if ((unsigned)p >= (unsigned)i) return i;                                       // a root (p == i); anything that is no smaller index ends the walk too
    i = p;
  }
}

// join the trees of the set pixels a and b; max(a, b) strictly decreases from one iteration to the next
template <int SCOPE>
__device__ __forceinline__ void cc_union(int* L, int a, int b) {
  for (;;) {
    a = cc_find<SCOPE>(L, a);
    b = cc_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
    if ((unsigned)old >= (unsigned)a || old == b) return;                           // a was a root and now points to b (or already did)
    a = old;                                                                        // someone lowered the slot first: join that parent with b
  }
}
