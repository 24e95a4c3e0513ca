// ack_args_check.cpp -- the device-free host half of the receive histories
// (ugo_amd/csrc/host/ack_args.hpp: the argument rules of every ugo_fec_ack_*
// entry point and the build of a set's member table) as a stand-alone program
// for AddressSanitizer + UBSan.  It needs no GPU and loads nothing else:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer tools/ack_args_check.cpp -o build/ack_args_check
//   UBSAN_OPTIONS=halt_on_error=1 ./build/ack_args_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ugo_amd/csrc/host/ack_args.hpp"

namespace {

int failures = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

using ugo::ackargs::Member;
namespace aa = ugo::ackargs;

void windows() {
  for (size_t wp : {size_t(0), size_t(1), size_t(512), size_t(1023), size_t(1025), size_t(1536), (size_t(1) << 20) + 1,
                    size_t(1) << 21, ~size_t(0)})
    EXPECT(!aa::window_ok(wp));
  for (size_t wp = 1024; wp <= (size_t(1) << 20); wp <<= 1) EXPECT(aa::window_ok(wp));
}

void members_and_table() {
  int ctx = 0, other = 0;
  const size_t n = 5000;
  std::vector<uint64_t> bits(n);  // stand-ins for device memory: only their addresses are used
  std::vector<ugo::kern::AckRecord> recs(n);
  std::vector<Member> ms(n);
  std::vector<const Member*> list(n);
  for (size_t i = 0; i < n; ++i) {
    ms[i] = Member{&ctx, &bits[i], &recs[i], size_t(1024) << (i % 11)};
    list[i] = &ms[i];
  }
  EXPECT(aa::members_ok(&ctx, list.data(), n));
  EXPECT(aa::members_ok(&ctx, list.data(), 1));
  EXPECT(!aa::members_ok(&ctx, list.data(), 0));
  EXPECT(!aa::members_ok(nullptr, list.data(), n));
  EXPECT(!aa::members_ok(&ctx, nullptr, n));
  EXPECT(!aa::members_ok(&ctx, list.data(), size_t(ugo::kern::kAckSetMaxConn) + 1));  // refused before a member is read
  EXPECT(!aa::members_ok(&other, list.data(), n));

  const std::vector<ugo::kern::AckEntry> t = aa::build_table(list.data(), n);
  EXPECT(t.size() == n);
  for (size_t i = 0; i < n; ++i)
    EXPECT(t[i].bits == &bits[i] && t[i].rec == &recs[i] && t[i].wp == (1024u << (i % 11)) && t[i].reserved == 0);

  std::mt19937_64 rng(0x5EED);
  for (int round = 0; round < 50; ++round) {
    std::vector<const Member*> l = list;
    std::shuffle(l.begin(), l.end(), rng);
    EXPECT(aa::members_ok(&ctx, l.data(), n));
    l[rng() % n] = l[0];  // l[0] a second time (or at 0 itself: then still fine)
    const bool dup = std::count(l.begin(), l.end(), l[0]) > 1;
    EXPECT(aa::members_ok(&ctx, l.data(), n) == !dup);
    l = list;
    l[rng() % n] = nullptr;
    EXPECT(!aa::members_ok(&ctx, l.data(), n));
  }
  Member foreign = ms[7];
  foreign.ctx = &other;
  std::vector<const Member*> l = list;
  l[7] = &foreign;
  EXPECT(!aa::members_ok(&ctx, l.data(), n));
  Member odd = ms[9];
  odd.window_packets = 3000;
  l = list;
  l[9] = &odd;
  EXPECT(!aa::members_ok(&ctx, l.data(), n));
}

void call_arguments() {
  alignas(16) unsigned char buf[256] = {};
  void* p = buf;
  void* off4 = buf + 4;
  void* off8 = buf + 8;
  void* off1 = buf + 1;
  EXPECT(aa::receive_ok(p, p, 4, nullptr, 0));
  EXPECT(aa::receive_ok(p, off4, size_t(1) << 31, off1, 0xffff));
  EXPECT(!aa::receive_ok(nullptr, p, 4, nullptr, 0));
  EXPECT(!aa::receive_ok(p, nullptr, 4, nullptr, 0));
  EXPECT(!aa::receive_ok(off8, p, 4, nullptr, 0));
  EXPECT(!aa::receive_ok(p, off1, 4, nullptr, 0));
  EXPECT(!aa::receive_ok(p, p, (size_t(1) << 31) + 1, nullptr, 0));
  EXPECT(!aa::receive_ok(p, p, 4, nullptr, 0x10000));
  EXPECT(!aa::receive_ok(p, p, 4, p, 0));

  EXPECT(aa::attach_ok(p, p, p, 4, p, p, 4, p, p, p));
  EXPECT(aa::attach_ok(off8, off4, off8, size_t(1) << 31, p, off8, 0xffff, off4, off8, off1));
  EXPECT(aa::attach_ok(p, p, p, 0, nullptr, nullptr, 4, nullptr, p, p));  // no packet slots: no arrays
  EXPECT(aa::attach_ok(p, p, p, 4, p, nullptr, 0, p, p, p));              // no range rows: no ranges
  EXPECT(!aa::attach_ok(nullptr, p, p, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, nullptr, p, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, nullptr, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, nullptr, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, nullptr, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 4, nullptr, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 4, p, nullptr, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 4, p, p, nullptr));
  EXPECT(!aa::attach_ok(off4, p, p, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, off1, p, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, off4, 4, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, off8, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, off4, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 4, off1, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 4, p, off4, p));
  EXPECT(!aa::attach_ok(p, p, p, (size_t(1) << 31) + 1, p, p, 4, p, p, p));
  EXPECT(!aa::attach_ok(p, p, p, 4, p, p, 0x10000, p, p, p));
}

}  // namespace

int main() {
  windows();
  members_and_table();
  call_arguments();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("ack_args_check ok");
  return 0;
}
