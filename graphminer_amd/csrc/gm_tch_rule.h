// gm_tch_rule.h -- which form of key addressing tch_kernel's flattened pass takes on a launch (gm_tch.hip).  Plain C++, no HIP: the
// rule is checked on the host by tests/tch_rule_host_check.cc.
//
// The flattened pass addresses a key with ONE vector add per tile: the descriptor of a list holds 4 * (key_base - its offset among the
// flattened positions) as a 32-bit byte offset (modulo 2^32), a lane adds 4 * lane + kTchFlatBias, and the load takes a scalar base
// (keys - bias + 4 * first position of the tile group) and the tile as its immediate offset.  key_base - offset may be negative (a list
// near the start of the array, late in its batch) while the index is not: the bias -- more than four bytes for every position a batch
// can have -- keeps the 32-bit sum from wrapping below zero, where its zero extension would be 4 GB off.
//
// RULE: that NARROW form is exact while 4 * index + bias + 256 < 2^32 for every index the pass can form, i.e. while THE ARRAY THE KEYS
// ARE STREAMED FROM has fewer than kTchNarrowEntries entries.  That array is col[] of the DAG (ne entries) -- or, on a handle whose
// short lists are streamed from their task-major copies (TaskLists::colk, gm_host.h: col[] followed by n_copy_keys copied keys, the
// descriptors pointing behind col[]), ne + n_copy_keys entries: GraphView::col_entries carries that extent beside the pointer.
// launch_tch starts the WIDE instance of the kernel (the index as an unsigned 32-bit sum, a 64-bit address per tile: exact for every
// index below 2^31) on any other launch.  Developer option GM_TCH_WIDE_NE lowers the limit (never raises it) so that tests reach
// the WIDE instance on small graphs.
#pragma once
#include <stdlib.h>

namespace gm {

constexpr unsigned kTchFlatBias = 1u << 17;
constexpr long long kTchNarrowEntries = (1ll << 30) - (long long)(kTchFlatBias >> 2) - 64;

// entries of the array a launch streams its keys from: col_entries where the view's col is longer than the DAG's own (0: it is not)
inline long long tch_key_entries(long long ne, long long col_entries) { return col_entries > ne ? col_entries : ne; }

// option: the value of GM_TCH_WIDE_NE or nullptr
inline bool tch_wide_form(long long key_entries, const char *option) {
  long long wide_from = kTchNarrowEntries;
  if (option) {
    long long v = atoll(option);
    if (v < 0) v = 0;
    if (v < wide_from) wide_from = v;
  }
  return key_entries >= wide_from;
}

}  // namespace gm
