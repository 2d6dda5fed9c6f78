// Ownership of device memory. A DeviceMem owns every allocation made through it (or adopted by it) and
// frees them in its destructor; an Arena stages several arrays into one allocation, each at a 256-byte
// aligned offset, with one upload. Every failing call leaves the pointers it was given null.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

namespace bos {
namespace dev {

// The backend: defined once in the library with HIP (device_mem.hip). host_mapped non-null: a
// host-mapped, coherent allocation (*host_mapped the host's address, *dev the device's).
bool dm_alloc(void** dev, size_t bytes, void** host_mapped);
void dm_free(void* dev, void* host_mapped);
bool dm_copy(void* dst, const void* src, size_t bytes);   // host to device
bool dm_zero(void* dst, size_t bytes);

class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    DeviceMem(DeviceMem&& o) noexcept { recs_.swap(o.recs_); }
    DeviceMem& operator=(DeviceMem&& o) noexcept {   // what this one held is freed
        if (this != &o) {
            clear();
            recs_.swap(o.recs_);
        }
        return *this;
    }
    ~DeviceMem() { clear(); }

    // count + pad elements (none, and a null pointer, for count 0); zero: all of them, otherwise the tail
    template <typename X> bool alloc(X** p, size_t count, bool zero, size_t pad = 0) {
        *p = nullptr;
        if (count == 0) return true;
        void* d = nullptr;
        const size_t bytes = (count + pad) * sizeof(X), head = zero ? 0 : count * sizeof(X);
        if (!dm_alloc(&d, bytes, nullptr)) return false;
        recs_.push_back({d, nullptr, bytes});
        if (bytes > head && !dm_zero(static_cast<char*>(d) + head, bytes - head)) return release(d), false;
        *p = static_cast<X*>(d);
        return true;
    }
    // an empty vector stays null, or (min_one) gets one element
    template <typename X> bool upload(X** p, const std::vector<X>& v, size_t pad = 0, bool min_one = false) {
        if (!alloc(p, v.empty() && min_one ? 1 : v.size(), false, pad)) return false;
        if (v.empty() || dm_copy(*p, v.data(), v.size() * sizeof(X))) return true;
        release(*p);
        *p = nullptr;
        return false;
    }
    // a pointer obtained elsewhere that the backend's free takes
    void adopt(void* p, size_t bytes) {
        if (p) recs_.push_back({p, nullptr, bytes});
    }
    // frees one allocation early (by its device or host address)
    void release(void* p) {
        for (size_t i = 0; p && i < recs_.size(); ++i)
            if (recs_[i].dev == p || recs_[i].host == p) {
                dm_free(recs_[i].dev, recs_[i].host);
                recs_.erase(recs_.begin() + i);
                return;
            }
    }
    // one zeroed X, host mapped
    template <typename X> bool host_mapped(X** host, X** dev) {
        void *d = nullptr, *h = nullptr;
        const bool ok = dm_alloc(&d, sizeof(X), &h);
        if (ok) {
            std::memset(h, 0, sizeof(X));
            recs_.push_back({d, h, sizeof(X)});
        }
        *host = static_cast<X*>(h);
        *dev = static_cast<X*>(d);
        return ok;
    }
    size_t bytes() const {
        size_t b = 0;
        for (const Rec& r : recs_) b += r.bytes;
        return b;
    }

private:
    struct Rec { void *dev, *host; size_t bytes; };
    std::vector<Rec> recs_;
    void clear() {
        for (const Rec& r : recs_) dm_free(r.dev, r.host);
        recs_.clear();
    }
};

// keep_empty false: an empty field takes no room and stays null; true: it takes one element's room
class Arena {
public:
    explicit Arena(bool keep_empty = false) : keep_empty_(keep_empty) {}
    template <typename X> void add(X** p, const X* src, size_t count) {
        const size_t off = field(p, count * sizeof(X), sizeof(X));
        stage(off, count * sizeof(X));
        if (count) std::memcpy(host_.data() + off, src, count * sizeof(X));
    }
    template <typename X> void add(X** p, const std::vector<X>& v) { add(p, v.data(), v.size()); }
    template <typename X> void zeros(X** p, size_t count) { stage(field(p, count * sizeof(X), sizeof(X)), count * sizeof(X)); }
    // an output-only region: not uploaded (zero only where a later field's upload passes over it)
    template <typename X> void reserve(X** p, size_t count) { field(p, count * sizeof(X), sizeof(X)); }
    size_t bytes() const { return bytes_; }
    // one allocation of bytes() and one upload; the fields then point into it
    bool commit(DeviceMem& m, char** base = nullptr) {
        char* a = nullptr;
        const bool ok = m.alloc(&a, bytes_, false) && place(a);
        if (!ok) m.release(a);
        if (base) *base = ok ? a : nullptr;
        return ok;
    }
    // the same into an allocation of at least bytes() that the caller holds
    bool place(char* a) {
        const bool ok = !a || host_.empty() || dm_copy(a, host_.data(), host_.size());
        for (const Field& f : fields_) *f.p = ok && a ? a + f.off : nullptr;
        return ok;
    }

private:
    struct Field { void** p; size_t off; };
    bool keep_empty_;
    size_t bytes_ = 0;
    std::vector<char> host_;   // the fields' data from offset 0 to the last uploaded field's end
    std::vector<Field> fields_;
    template <typename X> size_t field(X** p, size_t bytes, size_t elem) {
        *p = nullptr;
        if (bytes == 0 && !keep_empty_) return bytes_;
        fields_.push_back({reinterpret_cast<void**>(p), bytes_});
        bytes_ += ((bytes ? bytes : elem) + 255) / 256 * 256;
        return fields_.back().off;
    }
    void stage(size_t off, size_t n) {
        if (n) host_.resize(off + n, 0);
    }
};

}  // namespace dev
}  // namespace bos
