// The HIP backend of device_mem.hpp: the library's only calls that allocate or free device memory.
#include <hip/hip_runtime.h>

#include "device_mem.hpp"

namespace bos {
namespace dev {

bool dm_alloc(void** dev, size_t bytes, void** host_mapped) {
    *dev = nullptr;
    if (!host_mapped) {
        if (hipMalloc(dev, bytes) == hipSuccess) return true;
    } else if (hipHostMalloc(host_mapped, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
        if (hipHostGetDevicePointer(dev, *host_mapped, 0) == hipSuccess) return true;
        (void)hipHostFree(*host_mapped);
    }
    (void)hipGetLastError();
    *dev = nullptr;
    if (host_mapped) *host_mapped = nullptr;
    return false;
}

void dm_free(void* dev, void* host_mapped) {
    if (host_mapped) (void)hipHostFree(host_mapped);
    else if (dev) (void)hipFree(dev);
}

bool dm_copy(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; }

bool dm_zero(void* dst, size_t bytes) { return hipMemset(dst, 0, bytes) == hipSuccess; }

}  // namespace dev
}  // namespace bos
