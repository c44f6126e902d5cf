// css_devbuf.h -- an owning device buffer for the workspaces of css_index (css_index.hip).
#pragma once

#include "css_common.h"

#include <algorithm>
#include <utility>

namespace css {

// Pointer + capacity in ELEMENTS; the destructor frees, so the owner must die with its device current
// (css_index_free deletes the index inside its DeviceGuard).  Not copyable: a kernel launch takes `buf.p`, and
// handing it `buf` does not compile.  Growing never keeps the old contents.  Three policies, one per buffer:
//   grow        max(need, 2 x cap), failure is a hip_fail error: workspaces sized by the batch
//   grow_exact  exactly `need`, failure is a hip_fail error: buffers that can reach gigabytes or never grow again
//   try_exact   exactly `need`, failure is `false` with the HIP error cleared: the caller has a fallback
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)drop(); }

    hipError_t drop() {
        T* old = p;
        p = nullptr;
        cap = 0;
        return old ? hipFree(old) : hipSuccess;
    }
    T* release() {   // the caller owns the memory from here on
        T* old = p;
        p = nullptr;
        cap = 0;
        return old;
    }
    void swap(DevBuf& o) {   // (the row storage: built in locals, swapped in whole)
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    int grow(size_t need, const char* what = "hipMalloc(workspace)") {
        return need <= cap ? CSS_OK : alloc(std::max(need, cap * 2), what);
    }
    int grow_exact(size_t need, const char* what) { return need <= cap ? CSS_OK : alloc(need, what); }
    bool try_exact(size_t need) {
        if (need <= cap) return true;
        (void)drop();
        if (hipMalloc((void**)&p, need * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return false;
        }
        cap = need;
        return true;
    }

private:
    int alloc(size_t ncap, const char* what) {
        CSS_HIP_TRY(drop());
        const hipError_t e = hipMalloc((void**)&p, ncap * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return hip_fail(e, what, __FILE__, __LINE__);
        }
        cap = ncap;
        return CSS_OK;
    }
};

// a pair that is only useful whole: both at `need`, or both gone
template <typename A, typename B>
bool try_exact_pair(DevBuf<A>& a, DevBuf<B>& b, size_t need) {
    if (a.try_exact(need) && b.try_exact(need)) return true;
    (void)a.drop();
    (void)b.drop();
    return false;
}

}  // namespace css
