// gs_dyn_lds.cpp -- the opt-in for more than 64 KB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize), one table for
// every launcher of the step kernels' units (gs_kernels.h: gs_ensure_dyn_lds).
#include "gs_internal.h"
#include <mutex>

// The attribute belongs to the device function ON THE CURRENT DEVICE, so what has been set is remembered per (device,
// function): a process that drives several GPUs (device_ids = 0, 1, ...; two contexts) opts in on each.
// Contexts on different threads launch through here: the table has a lock, like tb_waves_of's.
static bool dyn_lds_seen(int device, const void *fn, int bytes, bool record)
{
    struct Entry { int device; const void *fn; int bytes; };
    static Entry table[256];
    static int n = 0;
    static std::mutex lock;
    std::lock_guard<std::mutex> guard(lock);
    for (int i = 0; i < n; ++i)
        if (table[i].device == device && table[i].fn == fn) {
            if (table[i].bytes >= bytes) return true;
            if (record) table[i].bytes = bytes;
            return false;
        }
    if (record && n < 256) table[n++] = Entry{device, fn, bytes};
    return false;
}
hipError_t gs_ensure_dyn_lds(const void *fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return hipSuccess;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    if (dyn_lds_seen(device, fn, (int)bytes, false)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) (void)dyn_lds_seen(device, fn, (int)bytes, true);
    return e;
}
// What the table above keys on, for the unit test of the key (tests/test_capi_cpu.py): 1 when (device, fn
// slot, bytes) is new, and it is recorded; 0 when a launch on that device would skip the call.
extern "C" int32_t gs_debug_dyn_lds_key(int32_t device, int32_t slot, int32_t bytes)
{
    static const char slots[16] = {0};
    if (slot < 0 || slot >= 16) return -1;
    if (dyn_lds_seen(-1000 - device, &slots[slot], bytes, false)) return 0;
    (void)dyn_lds_seen(-1000 - device, &slots[slot], bytes, true);
    return 1;
}
