// Error reporting and version entry points of libdss_hip.so.
#include <stdarg.h>
#include <atomic>
#include "common.h"

namespace dss {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Launch-error check (reference: AT_CUDA_CHECK(cudaGetLastError()), rasterize_points.cu:665).
// Does not synchronise.
int check_launch(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return DSS_ERR_LAUNCH;
    }
    return DSS_OK;
}

// Process-wide option table of dss_set_option: the ONLY mutable process state besides the thread-local error string.
// Relaxed atomics: an option is a tuning hint read once per call; callers change it between calls, not during one.
// Every option starts at 0 but DSS_OPT_FORWARD_FILL, which is set to 1 (write-through, include/dss_hip.h) when the library loads.
static std::atomic<int> g_opt[DSS_OPT_COUNT];
static const bool g_opt_defaults_set = (g_opt[DSS_OPT_FORWARD_FILL].store(1, std::memory_order_relaxed), true);
int option(int which) { return (which >= 0 && which < DSS_OPT_COUNT) ? g_opt[which].load(std::memory_order_relaxed) : 0; }

// Per-device cache of the CU count and of the resident workgroups per CU of the kernels whose persistent grids are sized by
// them (raster_backward.hip).  Lock-free: racing first callers compute and store the same values; a slot whose key is
// claimed but whose value is not stored yet reads as a miss.  Devices beyond DSS_MAX_DEVICES and kernels beyond a full
// table are queried on every call.
#define DSS_MAX_DEVICES 64
#define DSS_MAX_RESIDENT 64
struct DeviceCache {
    std::atomic<int> cus;
    std::atomic<const void *> kernel[DSS_MAX_RESIDENT];
    std::atomic<unsigned long long> value[DSS_MAX_RESIDENT];   // block << 32 | workgroups per CU; 0 = not stored yet
};
static DeviceCache g_dev[DSS_MAX_DEVICES];

int cu_count(int dev)
{
    DeviceCache *dc = (dev >= 0 && dev < DSS_MAX_DEVICES) ? &g_dev[dev] : nullptr;
    int cus = dc ? dc->cus.load(std::memory_order_relaxed) : 0;
    if (cus == 0) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
        if (dc) dc->cus.store(cus, std::memory_order_relaxed);
    }
    return cus;
}

unsigned resident_blocks(int dev, const void *kernel, int block)
{
    DeviceCache *dc = (dev >= 0 && dev < DSS_MAX_DEVICES) ? &g_dev[dev] : nullptr;
    int i = 0;
    for (; dc && i < DSS_MAX_RESIDENT; ++i) {
        const void *k = dc->kernel[i].load(std::memory_order_acquire);
        if (k == nullptr) break;
        const unsigned long long v = dc->value[i].load(std::memory_order_acquire);
        if (k == kernel && (v >> 32) == (unsigned)block) return (unsigned)v;
    }
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0);
    (void)hipGetLastError();
    if (per_cu < 1) per_cu = 1;
    const void *expect = nullptr;
    if (dc && i < DSS_MAX_RESIDENT && dc->kernel[i].compare_exchange_strong(expect, kernel, std::memory_order_acq_rel))
        dc->value[i].store((unsigned long long)block << 32 | (unsigned)per_cu, std::memory_order_release);
    return (unsigned)per_cu;
}

}  // namespace dss

extern "C" int dss_set_option(int option, int value)
{
    if (option < 0 || option >= DSS_OPT_COUNT) { dss::set_error("dss_set_option: unknown option %d", option); return DSS_ERR_INVALID_ARGUMENT; }
    if (option == DSS_OPT_BACKWARD_TPW && !(value == 0 || value == 1 || value == 2 || value == 4)) {
        dss::set_error("dss_set_option: DSS_OPT_BACKWARD_TPW takes 0 (automatic), 1, 2 or 4");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (option == DSS_OPT_BACKWARD_GRID && value < 0) {
        dss::set_error("dss_set_option: DSS_OPT_BACKWARD_GRID takes 0 (automatic) or a positive number of workgroups");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (option == DSS_OPT_MESH_LARGE && (value < 0 || value > 4096)) {
        dss::set_error("dss_set_option: DSS_OPT_MESH_LARGE takes 0 (default) or 1 .. 4096 quarters of a cell");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    if (option == DSS_OPT_FORWARD_FILL && !(value == 0 || value == 1)) {
        dss::set_error("dss_set_option: DSS_OPT_FORWARD_FILL takes 0 (plain stores) or 1 (write-through stores)");
        return DSS_ERR_INVALID_ARGUMENT;
    }
    dss::g_opt[option].store(value, std::memory_order_relaxed);
    return DSS_OK;
}
extern "C" int dss_get_option(int option) { return dss::option(option); }

// rows a band tensor has: the rows of [row0, row1) for a contiguous band; with row_cycle c > 1 the rows of every c-th
// 8-row tile row of [row0, row1), starting at row0
extern "C" int dss_band_rows(int row0, int row1, int row_cycle)
{
    if (row1 <= row0) return 0;
    if (row_cycle <= 1) return row1 - row0;
    const int span = row1 - row0, period = 8 * row_cycle;
    const int full = span / period, rem = span - full * period;
    return full * 8 + (rem < 8 ? rem : 8);
}

extern "C" int dss_version(void) { return DSS_HIP_VERSION; }
extern "C" const char *dss_last_error(void) { return dss::g_err; }
