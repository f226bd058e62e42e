// Host check of graphminer_amd/csrc/gm_orbit.h: the coefficient table of gm_orbits_from_noninduced rebuilt from first principles.
// For each of the six connected 4-vertex graphlets G and each vertex v of G, the non-induced counts N[4 .. 14] of v are taken by brute
// force -- every subset of G's edges that spans a connected graph on the four vertices is classified by its edge count and degree
// sequence, v by its degree inside it -- and the function must give back exactly the induced orbit of v in G, once.  The function is
// linear, so the eleven unit vectors pin every coefficient; a combination with multiplicities near 2^64 checks the wrap-around.
// Includes only that header; builds with a plain host compiler (and its sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../graphminer_amd/csrc/gm_orbit.h"

namespace {

struct Graphlet {
  const char *name;
  int ne;
  int e[6][2];
};
const Graphlet kGraphlets[6] = {
    {"4-path", 3, {{0, 1}, {1, 2}, {2, 3}}},
    {"3-star", 3, {{0, 1}, {0, 2}, {0, 3}}},
    {"4-cycle", 4, {{0, 1}, {1, 2}, {2, 3}, {3, 0}}},
    {"tailed triangle", 4, {{0, 1}, {1, 2}, {2, 0}, {0, 3}}},
    {"diamond", 5, {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {0, 2}}},
    {"4-clique", 6, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}},
};

// the orbit of vertex v in the spanning subgraph given by the edge mask of G; -1: the subgraph is not connected on four vertices
int orbit_of(const Graphlet &G, unsigned mask, int v) {
  int deg[4] = {0, 0, 0, 0}, m = 0;
  for (int i = 0; i < G.ne; ++i)
    if (mask >> i & 1u) {
      ++deg[G.e[i][0]];
      ++deg[G.e[i][1]];
      ++m;
    }
  int mn = 4, mx = 0;
  for (int d : deg) {
    mn = d < mn ? d : mn;
    mx = d > mx ? d : mx;
  }
  if (m < 3 || mn == 0) return -1;  // (three edges without an isolated vertex: a path or a star; a triangle leaves one isolated)
  const int d = deg[v];
  if (m == 3) return mx == 3 ? (d == 1 ? 6 : 7) : (d == 1 ? 4 : 5);
  if (m == 4) return mx == 2 ? 8 : (d == 1 ? 9 : d == 2 ? 10 : 11);
  if (m == 5) return d == 2 ? 12 : 13;
  return 14;
}

int fail(const char *what, const char *name, int v, int o, unsigned long long got, unsigned long long want) {
  std::printf("FAIL %s: %s vertex %d orbit %d: got %llu, want %llu\n", what, name, v, o, got, want);
  return 1;
}

}  // namespace

int main() {
  bool seen[kOrbits4] = {};
  uint64_t combo_N[kOrbits4] = {}, combo_o[kOrbits4] = {};
  uint64_t mult = 0x9E3779B97F4A7C15ull;  // (multiplicities of the combination: large, odd, different per case)
  for (const Graphlet &G : kGraphlets) {
    for (int v = 0; v < 4; ++v) {
      uint64_t N[kOrbits4] = {}, o[kOrbits4] = {};
      for (unsigned mask = 0; mask < (1u << G.ne); ++mask) {
        const int orb = orbit_of(G, mask, v);
        if (orb >= 0) ++N[orb];
      }
      const int own = orbit_of(G, (1u << G.ne) - 1u, v);
      if (own < 4) return fail("own orbit", G.name, v, own, 0, 0);
      seen[own] = true;
      gm_orbits_from_noninduced(N, o);
      for (int k = 0; k < kOrbits4; ++k)
        if (o[k] != (k == own ? 1ull : 0ull)) return fail("unit", G.name, v, k, o[k], k == own);
      for (int k = 0; k < kOrbits4; ++k) combo_N[k] += mult * N[k];
      combo_o[own] += mult;
      mult = mult * 6364136223846793005ull + 1442695040888963407ull;
    }
  }
  for (int k = 4; k < kOrbits4; ++k)
    if (!seen[k]) return fail("orbit never realised", "-", 0, k, 0, 1);
  // orbits 0 .. 3 pass through; the 4-vertex part wraps modulo 2^64
  combo_N[0] = 7, combo_N[1] = ~0ull, combo_N[2] = 1ull << 63, combo_N[3] = 12345;
  combo_o[0] = 7, combo_o[1] = ~0ull, combo_o[2] = 1ull << 63, combo_o[3] = 12345;
  uint64_t o[kOrbits4] = {};
  gm_orbits_from_noninduced(combo_N, o);
  for (int k = 0; k < kOrbits4; ++k)
    if (o[k] != combo_o[k]) return fail("combination", "-", 0, k, o[k], combo_o[k]);
  std::printf("orbit table ok\n");
  return 0;
}
