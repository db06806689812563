// Device memory one process exports and its z-neighbours map (HIP IPC): the buffers of the device-direct halo transport
// of tomobar_amd/slab.py.  Host code only; the copies in and out of a region are tomo_halo_pack2 / tomo_halo_pull2
// (glue_kernels.hip).  A region is an allocation of its own -- an IPC handle names a whole allocation, so memory carved out
// of a caching allocator's block cannot be exported on its own.
#include "tomo_common.h"

#include <cstring>

static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C-ABI carries an IPC handle as 64 opaque bytes");

// a failed IPC call must not leave its error behind for the next launch check of the calling thread
static int ipc_fail(hipError_t e, const char *what)
{
    (void)hipGetLastError();
    return tomo_fail(e == hipErrorOutOfMemory ? TOMO_E_NOMEM : TOMO_E_RUNTIME, "%s failed: %s", what, hipGetErrorString(e));
}

extern "C" int tomo_ipc_region_create(int device, size_t bytes, void **base_dev, unsigned char handle[64])
{
    TOMO_REQUIRE(base_dev != nullptr && handle != nullptr, "NULL output of tomo_ipc_region_create");
    TOMO_REQUIRE(bytes > 0, "an IPC region of 0 bytes");
    *base_dev = nullptr;
    TOMO_ON_DEVICE(device);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return ipc_fail(e, "hipMalloc of an IPC region");
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return ipc_fail(e, "hipIpcGetMemHandle");
    }
    std::memcpy(handle, &h, sizeof(h));
    *base_dev = p;
    return TOMO_OK;
}

extern "C" int tomo_ipc_region_open(int device, const unsigned char handle[64], void **mapped_dev)
{
    TOMO_REQUIRE(handle != nullptr && mapped_dev != nullptr, "NULL argument of tomo_ipc_region_open");
    *mapped_dev = nullptr;
    TOMO_ON_DEVICE(device);
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    void *p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess || p == nullptr) return ipc_fail(e == hipSuccess ? hipErrorUnknown : e, "hipIpcOpenMemHandle");
    *mapped_dev = p;
    return TOMO_OK;
}

extern "C" int tomo_ipc_region_close(void *mapped_dev)
{
    if (mapped_dev == nullptr) return TOMO_OK;
    hipError_t e = hipIpcCloseMemHandle(mapped_dev);
    if (e != hipSuccess) return ipc_fail(e, "hipIpcCloseMemHandle");
    return TOMO_OK;
}

extern "C" int tomo_ipc_region_destroy(void *base_dev)
{
    if (base_dev == nullptr) return TOMO_OK;
    hipError_t e = hipFree(base_dev);
    if (e != hipSuccess) return ipc_fail(e, "hipFree of an IPC region");
    return TOMO_OK;
}
