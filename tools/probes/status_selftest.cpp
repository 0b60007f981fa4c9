// Host-only self-test of csrc/bv_status.h: a stand-alone program that expands BV_DEFINE_STATUS the way a one-file
// library does and checks the message buffer under the address and undefined-behaviour sanitizers.  It never calls
// bv_check_launch, so it needs no device.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/probes/status_selftest.cpp -o status_selftest && ./status_selftest
#include <string.h>

#include <atomic>
#include <string>
#include <thread>

#define BV_STATUS_LINKAGE static
#include "../../big_vision_amd/csrc/bv_status.h"

BV_DEFINE_STATUS(selftest_last_error, selftest_version, 7)

static int require_positive(int x) {
  BV_REQUIRE(x > 0, "require_positive: got %d", x);
  return BV_OK;
}

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  CHECK(selftest_version() == 7 && strlen(selftest_last_error()) == 0);
  CHECK(require_positive(3) == BV_OK && strlen(selftest_last_error()) == 0);
  CHECK(require_positive(-4) == BV_ERR_INVALID_ARG && !strcmp(selftest_last_error(), "require_positive: got -4"));

  // an over-long message is cut at 511 characters plus the terminator
  const std::string big(2000, 'x');
  bv_set_error("%s", big.c_str());
  CHECK(strlen(selftest_last_error()) == 511 && std::string(selftest_last_error()) == big.substr(0, 511));
  bv_set_error("short");
  CHECK(!strcmp(selftest_last_error(), "short"));

  // every thread reads its own message; the pointers are those threads' buffers, read only while they live
  std::string seen[2];
  const char* where[2] = {nullptr, nullptr};
  std::atomic<int> done{0};
  std::thread t[2];
  for (int i = 0; i < 2; ++i)
    t[i] = std::thread([&, i] {
      for (int k = 0; k < 1000; ++k) {
        bv_set_error("thread %d round %d", i, k);
        where[i] = selftest_last_error();
        seen[i] = where[i];
      }
      done.fetch_add(1);                        // both buffers exist until both threads are through
      while (done.load() < 2) std::this_thread::yield();
    });
  for (auto& th : t) th.join();
  CHECK(seen[0] == "thread 0 round 999" && seen[1] == "thread 1 round 999");
  CHECK(where[0] != where[1] && where[0] != selftest_last_error() && where[1] != selftest_last_error());
  CHECK(!strcmp(selftest_last_error(), "short"));
  printf("status_selftest: ok\n");
  return 0;
}
