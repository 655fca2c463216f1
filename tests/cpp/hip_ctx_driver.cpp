// hip_ctx_driver.cpp -- what the compute contexts are made of (csrc/mgx_hip_util.h: resolve_device, pick_device, Owner, DevArray,
// PinBuf, Mirror) on a host without a HIP device, where every HIP call fails: the failure paths of a create.  Built with the
// host sanitizers and run by tests/test_hip_ctx_host.py with the devices hidden; exits 77 when it sees a device all the same.
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <utility>

#include "mgx_hip_util.h"

static int failures = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

using namespace mgx_hip;

static int resolve(int device, int n_dev, std::atomic<unsigned>* next, bool negative_is_zero, int* got) {
    *got = -99;
    return resolve_device(device, n_dev, next, negative_is_zero, got);
}

static void test_resolve_device() {
    int got;
    for (int d = 0; d < 3; ++d) { CHECK(resolve(d, 3, nullptr, false, &got) == 0 && got == d); }
    CHECK(resolve(3, 3, nullptr, false, &got) == -EINVAL && got == -99);
    CHECK(strstr(mgx_last_error(), "device 3 out of range (0..2)"));
    CHECK(resolve(-2, 3, nullptr, false, &got) == -EINVAL && got == -99);
    std::atomic<unsigned> a{0}, b{0};
    CHECK(resolve(-2, 3, &a, false, &got) == -EINVAL && a.load() == 0);
    for (int i = 0; i < 6; ++i) { CHECK(resolve(-1, 3, &a, false, &got) == 0 && got == i % 3); }
    CHECK(resolve(-1, 3, &b, false, &got) == 0 && got == 0);          // a counter of its own starts over
    CHECK(resolve(1, 3, &a, false, &got) == 0 && got == 1 && a.load() == 6);      // an explicit ordinal does not draw
    CHECK(resolve(-1, 3, nullptr, false, &got) == 0 && got == 0);
    CHECK(resolve(-7, 3, nullptr, true, &got) == 0 && got == 0);
    CHECK(resolve(-1, 3, nullptr, true, &got) == 0 && got == 0);
    CHECK(resolve(3, 3, nullptr, true, &got) == -EINVAL && got == -99);
    CHECK(resolve(0, 0, nullptr, false, &got) == -ENODEV && got == -99);
    CHECK(resolve(-1, 0, &a, false, &got) == -ENODEV && a.load() == 6);
    CHECK(strstr(mgx_last_error(), "no HIP device"));
}

static void test_pick_device() {
    std::atomic<unsigned> next{0};
    for (int asked : {0, -1, 5}) {
        int device = asked;
        mgx::set_error("none");
        CHECK(pick_device(&device, asked == -1 ? &next : nullptr) == -ENODEV);
        CHECK(strstr(mgx_last_error(), "no HIP device"));
        CHECK(device == asked);
    }
    int device = -4;
    CHECK(pick_device(&device, nullptr, true) == -ENODEV && device == -4);
}

// the first call of a create fails: every later one returns false as well, and nothing is held
enum First { kStream, kEvent, kPin, kDevice };
static void test_owner(First first) {
    static const char* const name[] = {"hipStreamCreate", "hipEventCreate", "hipHostMalloc", "hipMalloc"};
    Owner m;
    hipStream_t s = nullptr; hipEvent_t e = nullptr; char* h = nullptr; int* d = nullptr;
    CHECK(m.ok() && m.failed == nullptr);
    switch (first) {
        case kStream: CHECK(!m.stream(&s)); break;
        case kEvent: CHECK(!m.event(&e)); break;
        case kPin: CHECK(!m.pin(&h, 64)); break;
        case kDevice: CHECK(!m.device(&d, 64)); break;
    }
    CHECK(!m.ok() && m.failed && !strcmp(m.failed, name[first]));
    const hipError_t err = m.err;
    CHECK(!m.stream(&s) && !m.stream(&s, 256, 0x55u) && !m.stream(&s, 0, 0, true));
    CHECK(!m.event(&e) && !m.event(&e, hipEventDisableTiming));
    CHECK(!m.pin(&h, 64) && !m.device(&d, 64));
    CHECK(m.err == err && !strcmp(m.failed, name[first]));          // the first failure is the one kept
    CHECK(m.dev.empty() && m.pinned.empty() && m.events.empty() && m.streams.empty());
    m.release();
    m.release();
    CHECK(!m.ok());                                                  // release frees, it does not forgive
    m.reset();
    CHECK(m.ok() && m.failed == nullptr);
    CHECK(!m.device(&d, 64) && !strcmp(m.failed, "hipMalloc"));
}   // ... and the destructor releases once more

// reserve fails with -ENOMEM, leaves the object empty and may be called again; swap and move of such objects
template <typename A, typename Ptr>
static void test_array(Ptr A::*ptr) {
    A a;
    CHECK(a.reserve(0) == 0 && a.*ptr == nullptr && a.cap == 0);          // nothing to do: no HIP call
    CHECK(a.reserve(0, 64) == 0 && a.*ptr == nullptr && a.cap == 0);
    mgx::set_error("none");
    CHECK(a.reserve(100) == -ENOMEM && a.*ptr == nullptr && a.cap == 0);
    CHECK(strstr(mgx_last_error(), "failed"));
    CHECK(a.reserve(100, 125) == -ENOMEM && a.*ptr == nullptr && a.cap == 0);
    A b;
    a.swap(b);
    CHECK(a.*ptr == nullptr && a.cap == 0 && b.*ptr == nullptr && b.cap == 0);
    A c(std::move(a));
    CHECK(c.*ptr == nullptr && c.cap == 0 && a.*ptr == nullptr && a.cap == 0);
    b = std::move(c);
    A& self = b;
    b = std::move(self);
    CHECK(b.*ptr == nullptr && b.cap == 0);
    CHECK(b.reserve(7) == -ENOMEM && b.*ptr == nullptr && b.cap == 0);
    b.release();
    b.release();
}

int main() {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) { fprintf(stderr, "a HIP device is visible\n"); return 77; }
    (void)hipGetLastError();
    test_resolve_device();
    test_pick_device();
    for (First f : {kStream, kEvent, kPin, kDevice}) test_owner(f);
    test_array<DevArray<int>>(&DevArray<int>::p);
    test_array<PinBuf>(&PinBuf::p);
    test_array<Mirror>(&Mirror::dev);
    {
        Mirror m;
        CHECK(m.reserve(100) == -ENOMEM && m.dev == nullptr && m.pin == nullptr && m.cap == 0);
    }
    hipStream_t s = nullptr;
    CHECK(make_stream(&s) != hipSuccess && make_stream(&s, 256, 0x55u) != hipSuccess && make_stream(&s, 0, 0, true) != hipSuccess);
    (void)hipGetLastError();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("ok\n");
    fflush(stdout);      // the leak check at exit may end the process before stdio does
    return 0;
}
