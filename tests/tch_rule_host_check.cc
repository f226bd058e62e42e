// The rule that chooses tch_kernel's key addressing (graphminer_amd/csrc/gm_tch_rule.h), checked on the host:
//   g++ -std=c++17 -fsanitize=address,undefined tch_rule_host_check.cc
// The narrow form of the flattened pass adds, per lane, 4 * (key_base - off) (mod 2^32) + 4 * lane + bias as an unsigned 32-bit number to
// a 64-bit base of keys - bias + 4 * p0, plus 256 * q: the check forms exactly that sum for the extreme indices of an array of E entries
// and compares the address with &keys[index].  It must agree for every E the rule calls narrow, and the first E it calls wide is the first
// at which it can disagree by less than the safety margin; the extent of the array -- not the DAG's entry count -- decides.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../graphminer_amd/csrc/gm_tch_rule.h"

using namespace gm;

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #c);          \
      ++fails;                                               \
    }                                                        \
  } while (0)

// byte offset from keys[0] the narrow form addresses for: list at key_base, `off` flattened positions before it, position p0 + 64 q + lane
static int64_t narrow_offset(int64_t key_base, int64_t off, int64_t p0, int q, int lane) {
  const uint32_t dx = (uint32_t)((uint32_t)(int32_t)(key_base - off) << 2);  // the descriptor (kernel: (unsigned)(key_base - off) << 2)
  const uint32_t lane4 = ((uint32_t)lane << 2) + kTchFlatBias;
  const uint32_t voff = dx + lane4;                                          // ONE 32-bit vector add, zero-extended by the load
  return -(int64_t)kTchFlatBias + (p0 << 2) + (int64_t)voff + 256 * q;
}

int main() {
  const int64_t kPositions = 64 * 383;  // flattened positions of a batch at most (64 lists below kTchLongList = 384)
  CHECK((int64_t)kTchFlatBias >= 4 * (kPositions + 512));
  // ---- the arithmetic is exact on every array the rule calls narrow: the last list of the array, anywhere in its batch
  for (int64_t E : {(int64_t)1000, (int64_t)1 << 24, (int64_t)kTchNarrowEntries - 1}) {
    CHECK(!tch_wide_form(E, nullptr));
    for (int64_t len : {(int64_t)1, (int64_t)33, (int64_t)383}) {
      if (len > E) continue;
      const int64_t key_base = E - len;
      for (int64_t off : {(int64_t)0, (int64_t)1, (int64_t)255, kPositions - len}) {
        for (int64_t k : {(int64_t)0, len - 1}) {  // k-th key of the list sits at position off + k
          const int64_t p = off + k, p0 = (p / 256) * 256;
          const int q = (int)((p - p0) / 64), lane = (int)(p % 64);
          CHECK(narrow_offset(key_base, off, p0, q, lane) == 4 * (key_base + k));
        }
      }
    }
    // the first list of the array, late in its batch: key_base - off is negative, the index is not
    const int64_t off = kPositions - 40, p = off + 39, p0 = (p / 512) * 512;
    CHECK(narrow_offset(0, off, p0, (int)((p - p0) / 64), (int)(p % 64)) == 4 * 39);
  }
  // ---- and it is NOT on an array of 2^30 entries: what the rule keeps away
  {
    const int64_t E = (int64_t)1 << 30, key_base = E - 40;
    CHECK(narrow_offset(key_base, 0, 0, 0, 39) != 4 * (key_base + 39));
    CHECK(tch_wide_form(E, nullptr));
  }
  // ---- the threshold and the option's clamp
  CHECK(kTchNarrowEntries < ((int64_t)1 << 30) - (int64_t)(kTchFlatBias >> 2));
  CHECK(tch_wide_form(kTchNarrowEntries, nullptr) && !tch_wide_form(kTchNarrowEntries - 1, nullptr));
  CHECK(tch_wide_form(0, "0") && tch_wide_form(5, "5") && !tch_wide_form(4, "5"));
  CHECK(tch_wide_form(0, "-7"));                                         // negative: 0
  CHECK(tch_wide_form(kTchNarrowEntries, "2000000000"));                 // the option never raises the limit
  CHECK(!tch_wide_form(kTchNarrowEntries - 1, "2000000000"));
  // ---- the extent of the array streamed from decides, not the DAG's entry count
  const long long ne = 900000000ll, copies = 300000000ll;               // a DAG below the limit whose copies reach beyond it
  CHECK(!tch_wide_form(tch_key_entries(ne, 0), nullptr));
  CHECK(tch_wide_form(tch_key_entries(ne, ne + copies), nullptr));
  CHECK(tch_key_entries(ne, 0) == ne && tch_key_entries(ne, ne + copies) == ne + copies && tch_key_entries(ne, ne - 1) == ne);
  if (fails) return 1;
  printf("tch rule ok\n");
  return 0;
}
