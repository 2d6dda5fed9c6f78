// Stand-alone check of csrc/hip/device_mem.hpp (DeviceMem, Arena) on a malloc backend, built with
// -fsanitize=address,undefined by tests/test_device_mem_host.py: a leak, a double free or an
// out-of-bounds access ends the run with a report on stderr. The backend counts its calls so that the
// Nth allocation, copy or zeroing can be made to fail.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../prb-project-bearing-only-slam_amd/csrc/hip/device_mem.hpp"

static int g_calls = 0, g_fail_at = 0, g_live = 0;

namespace bos {
namespace dev {
static bool fails() { return ++g_calls == g_fail_at; }
bool dm_alloc(void** dev, size_t bytes, void** host_mapped) {
    *dev = nullptr;
    if (host_mapped) *host_mapped = nullptr;
    if (fails()) return false;
    *dev = std::malloc(bytes);
    if (host_mapped) *host_mapped = *dev;
    ++g_live;
    return true;
}
void dm_free(void* dev, void* host_mapped) {
    if (!dev && !host_mapped) return;
    std::free(host_mapped ? host_mapped : dev);
    --g_live;
}
bool dm_copy(void* dst, const void* src, size_t bytes) {
    if (fails()) return false;
    std::memcpy(dst, src, bytes);
    return true;
}
bool dm_zero(void* dst, size_t bytes) {
    if (fails()) return false;
    std::memset(dst, 0, bytes);
    return true;
}
}  // namespace dev
}  // namespace bos

using bos::dev::Arena;
using bos::dev::DeviceMem;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static bool aligned(const void* p, const void* base) { return ((const char*)p - (const char*)base) % 256 == 0; }

struct Status {
    int32_t seq;
    double chi2;
};

// Every operation the library's call sites use, in one owner. Returns false at the first failing call
// (only an injected failure can fail one), after checking that it left its pointers null.
static bool scenario() {
    DeviceMem m;
    // alloc, upload and pad tails
    double* a = (double*)1;
    if (!m.alloc(&a, 5, true, 3)) { CHECK(!a); return false; }
    for (int i = 0; i < 8; ++i) CHECK(a[i] == 0.0);
    int32_t* none = (int32_t*)1;
    CHECK(m.alloc(&none, 0, true, 7) && !none);
    const std::vector<int32_t> v = {1, 2, 3, 4, 5, 6, 7};
    int32_t* u = (int32_t*)1;
    if (!m.upload(&u, v, 64)) { CHECK(!u); return false; }
    for (size_t i = 0; i < v.size(); ++i) CHECK(u[i] == v[i]);
    for (size_t i = v.size(); i < v.size() + 64; ++i) CHECK(u[i] == 0);
    int16_t* tail = (int16_t*)1;
    if (!m.alloc(&tail, 3, false, 2)) { CHECK(!tail); return false; }
    tail[0] = tail[1] = tail[2] = 7;   // the body is the caller's; the tail is zero
    CHECK(tail[3] == 0 && tail[4] == 0);
    CHECK(m.bytes() == 8 * sizeof(double) + 71 * sizeof(int32_t) + 5 * sizeof(int16_t));
    // empty vectors: null, or one element with min_one
    const std::vector<int64_t> empty;
    int64_t *e0 = (int64_t*)1, *e1 = (int64_t*)1;
    CHECK(m.upload(&e0, empty) && !e0);
    if (!m.upload(&e1, empty, 0, true)) { CHECK(!e1); return false; }
    CHECK(e1);
    e1[0] = 42;
    // an arena: empty fields (dropped), a zeroed field, output-only regions and a final data field
    {
        const std::vector<double> x = {1.5, 2.5, 3.5};
        const std::vector<int32_t> y(100, 9), z = {4, 5};
        double *px = (double*)1, *out1 = (double*)1;
        int32_t *py = (int32_t*)1, *pz = (int32_t*)1, *pe = (int32_t*)1, *pzero = (int32_t*)1;
        char *out2 = (char*)1, *base = (char*)1;
        Arena ar;
        ar.add(&px, x);
        ar.add(&pe, std::vector<int32_t>());
        ar.add(&py, y);
        ar.zeros(&pzero, 70);
        ar.reserve(&out1, 33);
        ar.reserve(&out2, 1);
        ar.add(&pz, z.data(), z.size());
        CHECK(ar.bytes() == 256 + 512 + 512 + 512 + 256 + 256);
        if (!ar.commit(m, &base)) {
            CHECK(!px && !py && !pz && !pe && !pzero && !out1 && !out2 && !base);
            return false;
        }
        CHECK(!pe && (char*)px == base);
        CHECK(aligned(py, base) && aligned(pzero, base) && aligned(out1, base) && aligned(out2, base) && aligned(pz, base));
        CHECK(px < (double*)py && py < pzero && (char*)pzero < (char*)out1 && (char*)out1 < out2 && out2 < (char*)pz);
        CHECK(px[0] == 1.5 && px[2] == 3.5 && py[0] == 9 && py[99] == 9 && pz[0] == 4 && pz[1] == 5);
        for (int i = 0; i < 70; ++i) CHECK(pzero[i] == 0);
        out1[32] = 1.0;   // the regions are the caller's to write, to their last element
        out2[0] = 1;
        // the same layout again into the allocation the caller holds
        px = nullptr;
        if (!ar.place(base)) { CHECK(!px && !py && !pz); return false; }
        CHECK((char*)px == base && px[1] == 2.5);
    }
    {   // kept empty fields take one element's room and get a pointer
        int32_t *k0 = nullptr, *k1 = nullptr;
        double* k2 = nullptr;
        const int32_t one = 11;
        Arena ar(true);
        ar.add(&k0, (const int32_t*)nullptr, 0);
        ar.add(&k1, &one, 1);
        ar.reserve(&k2, 0);
        CHECK(ar.bytes() == 3 * 256);
        char* base = nullptr;
        if (!ar.commit(m, &base)) { CHECK(!k0 && !k1 && !k2 && !base); return false; }
        CHECK((char*)k0 == base && (char*)k1 == base + 256 && (char*)k2 == base + 512 && *k1 == 11);
        m.release(base);   // an arena's allocation freed early (a regrowth)
    }
    {   // an arena with nothing in it allocates nothing
        Arena ar;
        const int before = g_live;
        CHECK(ar.commit(m) && g_live == before && ar.bytes() == 0);
    }
    // adopt, release of a middle allocation, host-mapped pair
    void* foreign = nullptr;
    if (!bos::dev::dm_alloc(&foreign, 64, nullptr)) return false;
    m.adopt(foreign, 64);
    const size_t with_u = m.bytes();
    m.release(u);
    CHECK(m.bytes() == with_u - 71 * sizeof(int32_t));
    m.release(nullptr);
    Status *h = (Status*)1, *d = (Status*)1;
    if (!m.host_mapped(&h, &d)) { CHECK(!h && !d); return false; }
    CHECK(h->seq == 0 && h->chi2 == 0.0);
    d->seq = 3;
    CHECK(h->seq == 3);
    // move-assign into an owner that already holds allocations: they are freed, the source is left empty
    DeviceMem other;
    float* f = nullptr;
    if (!other.alloc(&f, 16, true)) { CHECK(!f); return false; }
    const int live = g_live;
    const size_t had = m.bytes();
    other = std::move(m);
    CHECK(g_live == live - 1 && other.bytes() == had && m.bytes() == 0);
    CHECK(a[0] == 0.0 && e1[0] == 42);   // still alive, in their new owner
    DeviceMem third(std::move(other));
    CHECK(third.bytes() == had && other.bytes() == 0);
    return true;
}

int main() {
    g_fail_at = 0;
    CHECK(scenario());
    CHECK(g_live == 0);
    const int calls = g_calls;
    CHECK(calls >= 15);
    for (int n = 1; n <= calls; ++n) {   // the Nth backend call fails: an error, null pointers, nothing leaked
        g_calls = 0;
        g_fail_at = n;
        CHECK(!scenario());
        CHECK(g_live == 0);
    }
    std::printf("device_mem_check: %d backend calls, every one failed in turn\n", calls);
    return 0;
}
