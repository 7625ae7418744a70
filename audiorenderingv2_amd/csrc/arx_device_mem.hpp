// arx_device_mem.hpp -- the two owners of the C ABI layer's memory (included by arx_internal.hpp, after
// ARX_HIP): DeviceBuf<T> for hipMalloc, PinnedBuf<T> for hipHostMalloc.  `cap` counts elements of T (T = char
// where the content is a byte layout) and is 0 exactly while there is no buffer.  Plain aggregates: no
// destructor, copied and reset by assignment like the structs that hold them; release is explicit, one list
// per owning struct next to its members.  Who must be idle before a buffer may be replaced differs per
// buffer and stays with the caller, in front of the reserve.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace arx {

// An optional buffer of `bytes` is not tried again once `no_room` bytes (> 0) did not fit on the device.
inline bool known_no_room(uint64_t no_room, uint64_t bytes) { return no_room > 0 && bytes >= no_room; }

template <class T>
struct DeviceBuf {
    T* p = nullptr;
    uint64_t cap = 0;
    uint64_t bytes() const { return cap * sizeof(T); }
    void release() {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // A buffer made elsewhere (widen_tree_arrays copies from the old one first) in place of this one.
    void adopt(T* q, uint64_t count) {
        release();
        p = q;
        cap = count;
    }
    // A buffer the call cannot do without: nothing while it holds `count` elements; else the old one freed,
    // then room for count + slack.  On failure there is no buffer.
    arx_status reserve(uint64_t count, uint64_t slack = 0) {
        if (p && count <= cap) return ARX_OK;
        release();
        ARX_HIP(hipMalloc(&p, (count + slack) * sizeof(T)));
        cap = count + slack;
        return ARX_OK;
    }
    // An optional buffer (the path cache, its filter, a batch's scratch).  False: no room on the device -- the
    // error cleared, no buffer, *no_room the bytes that did not fit; a size at or above *no_room is not tried
    // (and the old buffer stays).
    bool try_reserve(uint64_t count, uint64_t* no_room) {
        if (p && count <= cap) return true;
        if (known_no_room(*no_room, count * sizeof(T))) return false;
        release();
        if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            *no_room = count * sizeof(T);
            return false;
        }
        cap = count;
        return true;
    }
};

template <class T>
struct PinnedBuf {
    T* p = nullptr;
    uint64_t cap = 0;
    uint64_t bytes() const { return cap * sizeof(T); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    arx_status reserve(uint64_t count) {
        if (p && count <= cap) return ARX_OK;
        release();
        ARX_HIP(hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault));
        cap = count;
        return ARX_OK;
    }
};

}  // namespace arx
