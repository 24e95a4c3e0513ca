// sent_args_check.cpp -- the device-free host half of the sent histories
// (ugo_amd/csrc/host/sent_args.hpp: the argument rules of every ugo_fec_sent_*
// entry point, the layout of a history's device block and the build of a set's
// member and chunk tables) as a stand-alone program for AddressSanitizer +
// UBSan.  It needs no GPU and loads nothing else:
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer tools/sent_args_check.cpp -o build/sent_args_check
//   UBSAN_OPTIONS=halt_on_error=1 ./build/sent_args_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ugo_amd/csrc/host/sent_args.hpp"

namespace {

int failures = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

using ugo::sentargs::Member;
namespace sa = ugo::sentargs;

void windows_and_layout() {
  for (size_t ws : {size_t(0), size_t(1), size_t(512), size_t(1023), size_t(1025), size_t(1536), (size_t(1) << 20) + 1,
                    size_t(1) << 21, ~size_t(0)})
    EXPECT(!sa::window_ok(ws));
  for (size_t ws = 1024; ws <= (size_t(1) << 20); ws <<= 1) EXPECT(sa::window_ok(ws));
  EXPECT(!sa::seg_cap_ok(0) && !sa::seg_cap_ok(17) && sa::seg_cap_ok(1) && sa::seg_cap_ok(16));
  for (size_t ws = 1024; ws <= (size_t(1) << 20); ws <<= 1)
    for (size_t cap = 1; cap <= 16; ++cap) {
      const sa::Layout l = sa::layout(ws, cap);
      EXPECT(l.rec == 0 && l.slots >= sizeof(ugo_sent_state) && l.slots % 32 == 0 && l.segs == l.slots + ws * 32);
      EXPECT(l.segs % 16 == 0 && l.diff == l.segs + ws * cap * 16 && l.claim == l.diff + ws * 4);
      EXPECT(l.bytes == l.claim + ws * 4);
    }
}

void members_and_tables() {
  int ctx = 0, other = 0;
  const size_t n = 3000;
  std::vector<unsigned char> blocks(n * 64);  // stand-ins for device memory: only their addresses are used
  std::vector<Member> ms(n);
  std::vector<const Member*> list(n);
  for (size_t i = 0; i < n; ++i) {
    ms[i] = Member{&ctx, &blocks[i * 64], size_t(1024) << (i % 5), 1 + i % 16};
    list[i] = &ms[i];
  }
  EXPECT(sa::members_ok(&ctx, list.data(), n));
  EXPECT(sa::members_ok(&ctx, list.data(), 1));
  EXPECT(!sa::members_ok(&ctx, list.data(), 0));
  EXPECT(!sa::members_ok(nullptr, list.data(), n));
  EXPECT(!sa::members_ok(&ctx, nullptr, n));
  EXPECT(!sa::members_ok(&ctx, list.data(), size_t(ugo::kern::kSentSetMaxConn) + 1));  // refused before a member is read
  EXPECT(!sa::members_ok(&other, list.data(), n));

  std::vector<uint32_t> chunk_member;
  size_t min_cap = 0;
  const std::vector<ugo::kern::SentEntry> t = sa::build_table(list.data(), n, chunk_member, min_cap);
  EXPECT(t.size() == n && min_cap == 1);
  size_t chunks = 0;
  for (size_t i = 0; i < n; ++i) {
    const sa::Layout l = sa::layout(ms[i].window_packets, ms[i].seg_cap);
    EXPECT(reinterpret_cast<unsigned char*>(t[i].rec) == ms[i].block &&
           reinterpret_cast<unsigned char*>(t[i].slots) == ms[i].block + l.slots &&
           reinterpret_cast<unsigned char*>(t[i].segs) == ms[i].block + l.segs &&
           reinterpret_cast<unsigned char*>(t[i].diff) == ms[i].block + l.diff &&
           reinterpret_cast<unsigned char*>(t[i].claim) == ms[i].block + l.claim);
    EXPECT(t[i].ws == (1024u << (i % 5)) && t[i].seg_cap == 1 + i % 16 && t[i].chunk_base == chunks &&
           t[i].reserved == 0);
    for (size_t k = 0; k < ms[i].window_packets / 1024; ++k) EXPECT(chunk_member[chunks + k] == i);
    chunks += ms[i].window_packets / 1024;
  }
  EXPECT(chunk_member.size() == chunks);

  std::mt19937_64 rng(0x5EED);
  for (int round = 0; round < 30; ++round) {
    std::vector<const Member*> l = list;
    std::shuffle(l.begin(), l.end(), rng);
    EXPECT(sa::members_ok(&ctx, l.data(), n));
    l[rng() % n] = l[0];
    const bool dup = std::count(l.begin(), l.end(), l[0]) > 1;
    EXPECT(sa::members_ok(&ctx, l.data(), n) == !dup);
    l = list;
    l[rng() % n] = nullptr;
    EXPECT(!sa::members_ok(&ctx, l.data(), n));
  }
  std::vector<const Member*> l = list;
  Member foreign = ms[7];
  foreign.ctx = &other;
  l[7] = &foreign;
  EXPECT(!sa::members_ok(&ctx, l.data(), n));
  l = list;
  Member odd = ms[9];
  odd.window_packets = 3000;
  l[9] = &odd;
  EXPECT(!sa::members_ok(&ctx, l.data(), n));
  l = list;
  Member wide = ms[11];
  wide.seg_cap = 17;
  l[11] = &wide;
  EXPECT(!sa::members_ok(&ctx, l.data(), n));
  l = list;
  Member bare = ms[13];
  bare.block = nullptr;
  l[13] = &bare;
  EXPECT(!sa::members_ok(&ctx, l.data(), n));
}

void call_arguments() {
  alignas(16) unsigned char buf[256] = {};
  void* p = buf;
  void* off1 = buf + 1;
  void* off2 = buf + 2;
  void* off4 = buf + 4;
  void* off8 = buf + 8;
  EXPECT(sa::record_ok(p, p, 1, 1, p, p, p, 4));
  EXPECT(sa::record_ok(p, p, 16, 16, off4, off2, off1, size_t(1) << 31));
  EXPECT(!sa::record_ok(nullptr, p, 1, 1, p, p, p, 4) && !sa::record_ok(p, nullptr, 1, 1, p, p, p, 4));
  EXPECT(!sa::record_ok(p, p, 1, 1, nullptr, p, p, 4) && !sa::record_ok(p, p, 1, 1, p, nullptr, p, 4));
  EXPECT(!sa::record_ok(p, p, 1, 1, p, p, nullptr, 4));
  EXPECT(!sa::record_ok(off8, p, 1, 1, p, p, p, 4) && !sa::record_ok(p, off8, 1, 1, p, p, p, 4));
  EXPECT(!sa::record_ok(p, p, 1, 1, off2, p, p, 4) && !sa::record_ok(p, p, 1, 1, p, off1, p, 4));
  EXPECT(!sa::record_ok(p, p, 0, 1, p, p, p, 4) && !sa::record_ok(p, p, 5, 4, p, p, p, 4));
  EXPECT(!sa::record_ok(p, p, 1, 1, p, p, p, (size_t(1) << 31) + 1));

  EXPECT(sa::ack_ok(p, p, 4, p, 4, p));
  EXPECT(sa::ack_ok(nullptr, nullptr, 4, nullptr, 0, p));  // an empty batch still writes the event rows
  EXPECT(sa::ack_ok(p, nullptr, 0, p, 4, off8));
  EXPECT(!sa::ack_ok(p, p, 4, p, 4, nullptr) && !sa::ack_ok(nullptr, p, 4, p, 4, p));
  EXPECT(!sa::ack_ok(p, nullptr, 4, p, 4, p) && !sa::ack_ok(p, p, 4, nullptr, 4, p));
  EXPECT(!sa::ack_ok(off8, p, 4, p, 4, p) && !sa::ack_ok(p, off4, 4, p, 4, p) && !sa::ack_ok(p, p, 4, off2, 4, p));
  EXPECT(!sa::ack_ok(p, p, 4, p, 4, off4) && !sa::ack_ok(p, p, 0x10000, p, 4, p));
  EXPECT(!sa::ack_ok(p, p, 4, p, (size_t(1) << 31) + 1, p));

  EXPECT(sa::rto_ok(p, off1) && !sa::rto_ok(nullptr, p) && !sa::rto_ok(p, nullptr) && !sa::rto_ok(off4, p));

  EXPECT(sa::drain_ok(4, p, p, p, p, off1, p));
  EXPECT(sa::drain_ok(0, nullptr, nullptr, nullptr, p, p, p));
  EXPECT(!sa::drain_ok(4, nullptr, p, p, p, p, p) && !sa::drain_ok(4, p, nullptr, p, p, p, p));
  EXPECT(!sa::drain_ok(4, p, p, nullptr, p, p, p) && !sa::drain_ok(4, p, p, p, nullptr, p, p));
  EXPECT(!sa::drain_ok(4, p, p, p, p, nullptr, p) && !sa::drain_ok(4, p, p, p, p, p, nullptr));
  EXPECT(!sa::drain_ok(4, off2, p, p, p, p, p) && !sa::drain_ok(4, p, off4, p, p, p, p));
  EXPECT(!sa::drain_ok(4, p, p, off2, p, p, p) && !sa::drain_ok(4, p, p, p, off4, p, p));
  EXPECT(!sa::drain_ok(4, p, p, p, p, p, off4) && !sa::drain_ok((size_t(1) << 31) + 1, p, p, p, p, p, p));

  EXPECT(sa::attach_ok(p, p, 4, p, off1) && sa::attach_ok(off8, off4, 0, nullptr, p));
  EXPECT(!sa::attach_ok(nullptr, p, 4, p, p) && !sa::attach_ok(p, nullptr, 4, p, p));
  EXPECT(!sa::attach_ok(p, p, 4, nullptr, p) && !sa::attach_ok(p, p, 4, p, nullptr));
  EXPECT(!sa::attach_ok(off4, p, 4, p, p) && !sa::attach_ok(p, off2, 4, p, p) && !sa::attach_ok(p, p, 4, off8, p));
  EXPECT(!sa::attach_ok(p, p, (size_t(1) << 31) + 1, p, p));
}

}  // namespace

int main() {
  windows_and_layout();
  members_and_tables();
  call_arguments();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("sent_args_check ok");
  return 0;
}
