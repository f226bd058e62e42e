// gm_orbit.h -- the 15 graphlet-degree orbits of a vertex (3- and 4-vertex graphlets, Przulj's / ORCA's numbering) from its NON-INDUCED
// counts: N[o] = the edge-induced copies of orbit o's graphlet with the vertex in that position.  A copy of a graphlet spans an induced
// subgraph with at least its edges, so N is a triangular combination of the induced orbits o; the substitution runs from the 4-clique
// down.  The ONLY place the coefficients live: the finish kernel of gm_motif_local (gm_orbit_local.hip) includes it, and a plain host
// compiler builds it (tests/orbit_host_check.cc rebuilds every coefficient by brute force over the six 4-vertex graphlets).
// uint64 arithmetic modulo 2^64.  Needs nothing but <cstdint>.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GM_ORBIT_FN __host__ __device__ inline
#else
#define GM_ORBIT_FN inline
#endif

constexpr int kOrbits3 = 4, kOrbits4 = 15;

// N[0 .. 3] are the induced orbits 0 .. 3 themselves (degree, 2-path end, 2-path middle, triangle): they pass through.
GM_ORBIT_FN void gm_orbits_from_noninduced(const uint64_t (&N)[kOrbits4], uint64_t (&o)[kOrbits4]) {
  o[0] = N[0];
  o[1] = N[1];
  o[2] = N[2];
  o[3] = N[3];
  o[14] = N[14];
  o[13] = N[13] - 3 * o[14];
  o[12] = N[12] - 3 * o[14];
  o[11] = N[11] - 2 * o[13] - 3 * o[14];
  o[10] = N[10] - 2 * o[12] - 2 * o[13] - 6 * o[14];
  o[9] = N[9] - 2 * o[12] - 3 * o[14];
  o[8] = N[8] - o[12] - o[13] - 3 * o[14];
  o[7] = N[7] - o[11] - o[13] - o[14];
  o[6] = N[6] - o[9] - o[10] - 2 * o[12] - o[13] - 3 * o[14];
  o[5] = N[5] - 2 * o[8] - o[10] - 2 * o[11] - 2 * o[12] - 4 * o[13] - 6 * o[14];
  o[4] = N[4] - 2 * o[8] - 2 * o[9] - o[10] - 4 * o[12] - 2 * o[13] - 6 * o[14];
}
