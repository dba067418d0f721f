// Context-lifetime device memory: ctx_memory.h.
#include "ctx_memory.h"
#include "bugseg_internal.h"

namespace bugseg {

hipError_t CtxMemory::upload(std::initializer_list<HostSpan> spans, void **dev) {
    DeviceGuard g(device);
    RelaxCapture relax;
    hipStream_t s = setup_stream();
    size_t total = 0, off = 0;
    for (const HostSpan &h : spans) total += h.bytes;
    *dev = nullptr;
    hipError_t e = s ? hipMalloc(dev, total) : hipErrorInvalidValue;
    for (const HostSpan &h : spans) {
        if (e == hipSuccess) e = hipMemcpyAsync((unsigned char *)*dev + off, h.p, h.bytes, hipMemcpyHostToDevice, s);
        off += h.bytes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(*dev); *dev = nullptr; }
    return e;
}

}  // namespace bugseg
