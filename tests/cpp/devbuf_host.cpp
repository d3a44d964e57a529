// CPU: rpeh::DevBuf (csrc/rpe_devbuf.hpp) against a fake runtime.  The header includes no HIP header, so the six runtime names it uses
// are defined here over malloc / free, with a live-allocation count, a call log and a settable "fail the k-th call" for malloc, copy
// and wait.  Built with -fsanitize=address,undefined and leak detection on: nothing here links the HIP runtime.
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// ---- the fake runtime
typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum { hipMemcpyDeviceToDevice = 3 };
enum { RPE_OK = 0, RPE_ERR_HIP = -3 };

static int g_live = 0;                       // allocations not yet freed
static std::string g_log;                    // one letter per runtime call: m(alloc) f(ree) c(opy) w(ait)
static int g_fail_malloc = 0, g_fail_copy = 0, g_fail_wait = 0;   // k > 0: the k-th call from now fails (once)
static bool trip(int* k) { return *k > 0 && --*k == 0; }

static hipError_t hipMalloc(void** p, size_t bytes) {
  g_log += 'm';
  assert(bytes > 0);
  if (trip(&g_fail_malloc)) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes);
  g_live++;
  return hipSuccess;
}
static hipError_t hipFree(void* p) { g_log += 'f'; assert(p); std::free(p); g_live--; return hipSuccess; }
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, int kind, hipStream_t) {
  g_log += 'c';
  assert(kind == hipMemcpyDeviceToDevice);
  if (trip(&g_fail_copy)) return hipErrorUnknown;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t) { g_log += 'w'; return trip(&g_fail_wait) ? hipErrorUnknown : hipSuccess; }
static const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "unknown error"; }

#include "../../rgbd_pose_estimation_amd/csrc/rpe_devbuf.hpp"

static std::string g_err;
namespace rpeh {
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace rpeh
using rpeh::DevBuf;
using rpeh::DevMem;

struct Ctx { hipStream_t stream = nullptr; };
#define CHECK(x) do { if (!(x)) { std::printf("devbuf_host: FAILED %s (line %d; log '%s', error '%s')\n", #x, __LINE__, g_log.c_str(), g_err.c_str()); return 1; } } while (0)

static void fill(unsigned char* p, size_t n, unsigned seed) { for (size_t i = 0; i < n; i++) p[i] = (unsigned char)(seed * 131 + i * 7 + (i >> 8)); }

// regrow over N buffers (buffer i: 40 + 8 i bytes, of which 16 + 4 i are kept, to 100 + 10 i): once clean, then with the failure
// injected at every single malloc, every single copy and the wait in turn
template <size_t N> static int regrow_case(Ctx* c) {
  for (int inject = 0; inject <= 2 * (int)N + 1; inject++) {   // 0: none; 1 .. N: malloc; N + 1 .. 2 N: copy; 2 N + 1: the wait
    DevBuf<unsigned char> b[N];
    std::vector<std::vector<unsigned char>> was(N);
    DevMem::Grow g[N];
    for (size_t i = 0; i < N; i++) {
      CHECK(b[i].reserve(c, 40 + 8 * i) == RPE_OK);
      fill(b[i], 40 + 8 * i, (unsigned)i + 1);
      was[i].assign(b[i].get(), b[i].get() + 40 + 8 * i);
      g[i] = DevMem::Grow{&b[i], 16 + 4 * i, 100 + 10 * i};
    }
    void* ptr[N]; size_t cap[N];
    for (size_t i = 0; i < N; i++) { ptr[i] = b[i].get(); cap[i] = b[i].bytes(); }
    const int live = g_live;
    g_fail_malloc = inject >= 1 && inject <= (int)N ? inject : 0;
    g_fail_copy = inject > (int)N && inject <= 2 * (int)N ? inject - (int)N : 0;
    g_fail_wait = inject == 2 * (int)N + 1 ? 1 : 0;
    g_log.clear(); g_err.clear();
    const int rc = DevMem::regrow(c, "test storage", g);
    CHECK(g_fail_malloc == 0 && g_fail_copy == 0 && g_fail_wait == 0);   // the injected failure was reached
    if (inject == 0) {
      CHECK(rc == RPE_OK);
      CHECK(g_log == std::string(N, 'm') + std::string(N, 'c') + "w" + std::string(N, 'f'));   // new arrays, copies, ONE wait, old arrays go
      CHECK(g_live == live);
      for (size_t i = 0; i < N; i++) {
        CHECK(b[i].get() != nullptr && b[i].bytes() == 100 + 10 * i);
        CHECK(std::memcmp(b[i].get(), was[i].data(), 16 + 4 * i) == 0);      // the kept prefix, byte for byte
        std::memset(b[i].get(), 0xEE, 100 + 10 * i);                         // (the whole new array is ours to write)
      }
    } else {
      CHECK(rc == RPE_ERR_HIP && g_err.rfind("test storage: ", 0) == 0);     // the caller's wording
      CHECK(g_live == live);
      for (size_t i = 0; i < N; i++) {
        CHECK(b[i].get() == ptr[i] && b[i].bytes() == cap[i]);
        CHECK(std::memcmp(b[i].get(), was[i].data(), was[i].size()) == 0);
      }
    }
  }
  return 0;
}

namespace { struct Holder { DevBuf<float> z; DevBuf<unsigned int> rgba; bool have = false; int tag = 0; }; }

static int run() {
  Ctx ctx, *c = &ctx;
  {  // reserve: enough room = no runtime call; larger = wait, free, malloc; capacity = the bytes asked
    DevBuf<int> b;
    CHECK(!b && b.bytes() == 0);
    CHECK(b.reserve(c, 64) == RPE_OK && g_log == "m" && b && b.bytes() == 64 && g_live == 1);
    int* const p = b;
    g_log.clear();
    CHECK(b.reserve(c, 64) == RPE_OK && b.reserve(c, 10) == RPE_OK && b.reserve(c, 0) == RPE_OK);
    CHECK(g_log.empty() && b.get() == p && b.bytes() == 64);
    CHECK(b.reserve(c, 65) == RPE_OK && g_log == "wfm" && b.bytes() == 65 && g_live == 1);
    // a failed malloc leaves it empty with capacity 0; the next reserve succeeds
    g_log.clear(); g_fail_malloc = 1;
    CHECK(b.reserve(c, 200) == RPE_ERR_HIP && g_log == "wfm" && !b && b.bytes() == 0 && g_live == 0);
    CHECK(g_err.find("out of memory") != std::string::npos);
    g_log.clear();
    CHECK(b.reserve(c, 200) == RPE_OK && g_log == "m" && b && b.bytes() == 200 && g_live == 1);
    // a failed wait leaves it as it was
    int* const p2 = b;
    g_fail_wait = 1;
    CHECK(b.reserve(c, 300) == RPE_ERR_HIP && b.get() == p2 && b.bytes() == 200 && g_live == 1);
  }
  CHECK(g_live == 0);
  {  // zero bytes on an empty buffer: still a pointer; once: only when empty
    DevBuf<short> b;
    CHECK(b.reserve(c, 0) == RPE_OK && b.get() != nullptr && b.bytes() == 0 && g_live == 1);
    CHECK(b.reserve(c, 2) == RPE_OK && b.bytes() == 2 && g_live == 1);
    DevBuf<void> o;
    g_log.clear();
    CHECK(o.once(c, 32) == RPE_OK && g_log == "m" && o.bytes() == 32);
    void* const p = o;
    CHECK(o.once(c, 4096) == RPE_OK && g_log == "m" && o.get() == p && o.bytes() == 32);
    g_fail_malloc = 1;
    DevBuf<void> f;
    CHECK(f.once(c, 8) == RPE_ERR_HIP && !f && f.bytes() == 0);
    CHECK(f.once(c, 8) == RPE_OK && f);
    // move: the source is empty afterwards, the target's old array goes
    DevBuf<void> m(std::move(o));
    CHECK(!o && o.bytes() == 0 && m.get() == p && m.bytes() == 32);
    const int live = g_live;
    f = std::move(m);
    CHECK(g_live == live - 1 && f.get() == p && !m);
    f = {};
    CHECK(g_live == live - 2 && !f && f.bytes() == 0);
  }
  CHECK(g_live == 0);
  if (regrow_case<1>(c) || regrow_case<3>(c) || regrow_case<5>(c)) return 1;
  CHECK(g_live == 0);
  {  // regrow of buffers that are still empty: nothing to copy, nothing to free
    DevBuf<int> a, b;
    const DevMem::Grow g[] = {{&a, 0, 24}, {&b, 16, 48}};
    g_log.clear();
    CHECK(DevMem::regrow(c, "test storage", g) == RPE_OK && g_log == "mmw" && a.bytes() == 24 && b.bytes() == 48 && g_live == 2);
  }
  CHECK(g_live == 0);
  {  // a vector of structs that hold buffers: up (reallocating, so every element moves), down, up again -- no double free, no leak
    std::vector<Holder> v;
    v.resize(3);
    for (int i = 0; i < 3; i++) { CHECK(v[i].z.reserve(c, 16 * (i + 1)) == RPE_OK); v[i].tag = i; }
    float* const z1 = v[1].z;
    v.resize(v.capacity() + 50);
    CHECK(g_live == 3 && v[1].z.get() == z1 && v[1].z.bytes() == 32 && v[1].tag == 1 && !v[40].z);
    CHECK(v[40].rgba.reserve(c, 8) == RPE_OK && g_live == 4);
    v.resize(2);
    CHECK(g_live == 2);
    v.resize(6);
    CHECK(g_live == 2 && v[0].z && !v[2].z);
  }
  CHECK(g_live == 0);
  return 0;
}

int main() {
  if (run()) return 1;
  if (g_live != 0) { std::printf("devbuf_host: FAILED %d allocation(s) still live at exit\n", g_live); return 1; }
  std::printf("devbuf_host: ok\n");
  return 0;
}
