// csrc/dss_core.cpp -- errors, device selection and the version string of libdss_hip.so (include/dss_hip.h).
#include <stdarg.h>
#include <stdlib.h>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// errors / device
// ------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void dss_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *dss_last_error(void) { return g_err; }

static thread_local int g_device = -1;

int dss_ensure_device(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        dss_set_error("no HIP device available (%s); libdss_hip has no CPU fallback",
                      e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return DSS_ENODEV;
    }
    if (g_device < 0) {
        const char *lr = getenv("LOCAL_RANK");
        int d = lr ? atoi(lr) : 0;
        g_device = (d >= 0 && d < n) ? d : 0;
    }
    DSS_HIP_CHECK(hipSetDevice(g_device));
    return DSS_OK;
}

extern "C" int dss_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int dss_set_device(int device)
{
    int n = dss_device_count();
    if (device < 0 || device >= n) { dss_set_error("device %d out of range (%d devices)", device, n); return DSS_EINVAL; }
    g_device = device;
    DSS_HIP_CHECK(hipSetDevice(device));
    return DSS_OK;
}

extern "C" int dss_current_device(void)
{
    if (dss_ensure_device()) return DSS_ENODEV;
    return g_device;
}

extern "C" const char *dss_version(void)
{
    static char buf[256];
    hipDeviceProp_t p;
    int n = dss_device_count();
    if (n > 0 && hipGetDeviceProperties(&p, g_device < 0 ? 0 : g_device) == hipSuccess)
        snprintf(buf, sizeof(buf), "libdss_hip 0.1 (gfx950 build) on %s %s, %d CUs", p.name, p.gcnArchName, p.multiProcessorCount);
    else
        snprintf(buf, sizeof(buf), "libdss_hip 0.1 (gfx950 build), no device");
    return buf;
}
