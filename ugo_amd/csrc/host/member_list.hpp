// member_list.hpp -- the member rule every set create of the C ABI shares: at
// least one member, none NULL, all of the set's context, none listed twice.
// Needs no device and no HIP, so that a stand-alone program can run it under a
// sanitizer (tools/member_list_check.cpp), as host/ack_args.hpp is.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace ugo {
namespace members __attribute__((visibility("hidden"))) {  // libugofec.so exports the C ABI, not its plumbing

// M is anything with a `ctx` member: a handle, or the ackargs / sentargs view of one.  A member listed
// twice would get two table entries over one record.  The sorted copy may throw std::bad_alloc.
template <class M>
bool list_ok(const void* ctx, M* const* members, size_t nconn) {
  if (!ctx || !members || nconn == 0) return false;
  for (size_t i = 0; i < nconn; ++i)
    if (!members[i] || members[i]->ctx != ctx) return false;
  std::vector<const void*> sorted(members, members + nconn);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

}  // namespace members
}  // namespace ugo
