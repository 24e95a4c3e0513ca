// member_list_check.cpp -- the member rule every set create of the C ABI shares
// (ugo_amd/csrc/host/member_list.hpp: at least one member, none NULL, all of the
// set's context, none listed twice) as a stand-alone program for
// AddressSanitizer + UBSan.  It needs no GPU and loads nothing else:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer tools/member_list_check.cpp -o build/member_list_check
//   UBSAN_OPTIONS=halt_on_error=1 ./build/member_list_check
#include <cstdio>
#include <random>
#include <vector>

#include "../ugo_amd/csrc/host/member_list.hpp"

namespace {

int failures = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

struct Handle {  // what list_ok asks of a member: a context
  const void* ctx;
};
using ugo::members::list_ok;

std::vector<Handle*> pointers(std::vector<Handle>& hs) {
  std::vector<Handle*> l(hs.size());
  for (size_t i = 0; i < hs.size(); ++i) l[i] = &hs[i];
  return l;
}

void small_lists() {
  int ctx = 0, other = 0;
  std::vector<Handle> hs(5, Handle{&ctx});
  std::vector<Handle*> l = pointers(hs);
  EXPECT(list_ok(&ctx, l.data(), 5));
  EXPECT(list_ok(&ctx, l.data(), 1));
  EXPECT(!list_ok(&ctx, l.data(), 0));  // an empty list
  EXPECT(!list_ok(&ctx, static_cast<Handle* const*>(nullptr), 5));
  EXPECT(!list_ok(nullptr, l.data(), 5));
  EXPECT(!list_ok(&other, l.data(), 5));  // every member foreign
  for (size_t k = 0; k < 5; ++k) {        // a NULL member, a foreign one, at every place
    std::vector<Handle*> m = l;
    m[k] = nullptr;
    EXPECT(!list_ok(&ctx, m.data(), 5));
    Handle foreign{&other};
    m[k] = &foreign;
    EXPECT(!list_ok(&ctx, m.data(), 5));
  }
  std::vector<Handle*> ends = l, middle = l, pair = {l[0], l[0]};
  ends[4] = ends[0];  // a duplicate at the ends
  middle[3] = middle[2];  // and in the middle
  EXPECT(!list_ok(&ctx, ends.data(), 5));
  EXPECT(!list_ok(&ctx, middle.data(), 5));
  EXPECT(!list_ok(&ctx, pair.data(), 2));
  EXPECT(list_ok(&ctx, ends.data(), 4));  // the prefix without the repeat is a set
  // a view of a handle is const (host/ack_args.hpp's Member): the same rule
  std::vector<const Handle*> views(l.begin(), l.end());
  EXPECT(list_ok(&ctx, views.data(), 5));
  views[1] = views[4];
  EXPECT(!list_ok(&ctx, views.data(), 5));
}

void large_list() {
  int ctx = 0;
  const size_t n = 32769;
  std::vector<Handle> hs(n, Handle{&ctx});
  std::vector<Handle*> l = pointers(hs);
  std::mt19937_64 rng(0x5EED);
  std::shuffle(l.begin(), l.end(), rng);
  const std::vector<Handle*> before = l;
  EXPECT(list_ok(&ctx, l.data(), n));
  EXPECT(l == before);  // the caller's list is read, never reordered
  std::vector<Handle*> m = l;
  m[n - 1] = m[0];
  EXPECT(!list_ok(&ctx, m.data(), n));
  m = l;
  m[n / 2] = m[n / 2 - 1];
  EXPECT(!list_ok(&ctx, m.data(), n));
}

}  // namespace

int main() {
  small_lists();
  large_list();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("member_list_check ok");
  return 0;
}
