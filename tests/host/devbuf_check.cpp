// Host-only check of csrc/cnf_devbuf.h against a stubbed allocator: every allocation is freed exactly once and with the matching
// call, reserve() is grow-only and makes no call when the buffer is large enough, a failed allocation leaves the buffer empty, and
// moves transfer ownership.  Compiled and run by tests/test_devbuf_host.py; needs no GPU and no HIP runtime library.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "cnf_devbuf.h"

static std::map<void*, int> g_live;   // pointer -> 0 device, 1 pinned
static int g_calls = 0, g_bad = 0;
static size_t g_fail_above = ~(size_t)0;

static hipError_t stub_alloc(void** p, size_t bytes, int kind) {
    ++g_calls;
    if (bytes > g_fail_above) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    g_live[*p] = kind;
    return hipSuccess;
}
static hipError_t stub_free(void* p, int kind) {
    ++g_calls;
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) { ++g_bad; return hipErrorInvalidValue; }
    g_live.erase(it);
    std::free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return stub_alloc(p, n, 0); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return stub_alloc(p, n, 1); }
hipError_t hipFree(void* p) { return stub_free(p, 0); }
hipError_t hipHostFree(void* p) { return stub_free(p, 1); }
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

struct Holder { cnf::DevBuf<float> a; cnf::PinnedBuf<int> b; int tag = 0; };

int main() {
    using cnf::DevBuf;
    {
        DevBuf<float> b;
        bool grew = true;
        CHECK(b.data() == nullptr && b.capacity() == 0 && !b);
        CHECK(b.reserve(0, &grew) == hipSuccess && !grew && g_calls == 0);          // nothing asked, nothing done
        CHECK(b.reserve(100, &grew) == hipSuccess && grew && b.capacity() == 100 && b.data());
        float* first = b;
        first[99] = 1.f;                                                            // 100 floats are really there
        const int calls = g_calls;
        CHECK(b.reserve(100, &grew) == hipSuccess && !grew && g_calls == calls);    // large enough: no call at all
        CHECK(b.reserve(7, &grew) == hipSuccess && !grew && g_calls == calls && b.data() == first && b.capacity() == 100);
        CHECK(b.reserve(101, &grew) == hipSuccess && grew && b.capacity() == 101 && g_live.size() == 1);   // the old block went first
        g_fail_above = 1000;
        CHECK(b.reserve(1000, &grew) == hipErrorOutOfMemory && grew);               // a failed growth leaves an empty buffer ...
        CHECK(b.data() == nullptr && b.capacity() == 0 && g_live.empty());
        g_fail_above = ~(size_t)0;
        CHECK(b.reserve(10) == hipSuccess && b.capacity() == 10);                   // ... that can be used again
        b.release();
        CHECK(b.data() == nullptr && b.capacity() == 0 && g_live.empty());
        b.release();                                                                // twice is harmless
        CHECK(g_bad == 0);
    }
    {
        DevBuf<double> a, c;
        CHECK(a.reserve(5) == hipSuccess && c.reserve(6) == hipSuccess && g_live.size() == 2);
        double* pa = a;
        DevBuf<double> m(std::move(a));
        CHECK(m.data() == pa && m.capacity() == 5 && a.data() == nullptr && a.capacity() == 0);
        c = std::move(m);                                                           // c's own block is freed, m's taken over
        CHECK(c.data() == pa && c.capacity() == 5 && m.data() == nullptr && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_bad == 0);
    {
        std::vector<Holder> v;                                                      // as LayeredGrad::images: growth moves the elements
        for (int i = 0; i < 40; ++i) {
            Holder h;
            h.tag = i;
            CHECK(h.a.reserve(i + 1) == hipSuccess);
            if (i % 3 == 0) CHECK(h.b.reserve(4) == hipSuccess);                    // used and unused members side by side
            v.push_back(std::move(h));
        }
        for (int i = 0; i < 40; ++i)
            CHECK(v[i].tag == i && v[i].a.capacity() == (size_t)i + 1 && (v[i].b.data() != nullptr) == (i % 3 == 0));
        CHECK(g_live.size() == 40 + 14);
        Holder* h = new Holder();
        CHECK(h->b.reserve(3) == hipSuccess);
        delete h;                                                                   // pinned memory goes back through hipHostFree
        CHECK(g_bad == 0 && g_live.size() == 40 + 14);
    }
    CHECK(g_live.empty() && g_bad == 0);
    std::printf("devbuf ok: %d allocator calls\n", g_calls);
    return 0;
}
