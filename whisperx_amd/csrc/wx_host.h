// wx_host.h — host helpers the entry points share: the launch epilogue and the workspace carver.
#ifndef WX_HOST_H
#define WX_HOST_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wx_align.h"

namespace wx {
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int launch_status() {  // WX_OK, or the HIP error the launches before it left behind
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? WX_OK : (int)e;
}

// Bump carver: take<T>(n) is the next region of n elements, padded to 256 bytes.  A workspace's one
// carving function states its layout once and returns `off`, the bytes taken: on a null base it only
// measures (pointers from null, never to be used), on the caller's pointer it fills the kernels' arguments.
struct Carver {
    void* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off);
        off += align_up(count * sizeof(T), 256);
        return p;
    }
};
}  // namespace wx
#endif  // WX_HOST_H
