// Device memory that lives as long as a context (host only). DESIGN.md 6.26 states its lifetime rules.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

namespace bugseg {

// `stream` is being captured into a graph, or its state cannot be read (the legacy stream while another captures).
inline bool stream_capturing(void *stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
}

// Lets this thread allocate and wait on the setup stream while one of its streams captures in the global mode.
struct RelaxCapture {
    hipStreamCaptureMode m = hipStreamCaptureModeRelaxed;
    RelaxCapture() { (void)hipThreadExchangeStreamCaptureMode(&m); }
    ~RelaxCapture() { (void)hipThreadExchangeStreamCaptureMode(&m); }
};

struct HostSpan { const void *p; size_t bytes; };

// The caller of every member but upload has made `device` current.
class CtxMemory {
public:
    const int device;                   // the context's HIP device
    explicit CtxMemory(int dev) : device(dev) {}
    ~CtxMemory() {                      // (the owner has synchronised; a host-only context makes no HIP call)
        for (void *p : graveyard) (void)hipFree(p);
        if (setup) (void)hipStreamDestroy(setup);
    }
    hipStream_t setup_stream() {        // private, non-blocking, created on first use (null: it could not be)
        if (!setup && hipStreamCreateWithFlags(&setup, hipStreamNonBlocking) != hipSuccess) setup = nullptr;
        return setup;
    }
    // Free memory that enqueued work may still read: device sync + free, or, while capturing, the graveyard.
    void retire(void *p, bool capturing) {
        if (p && capturing) graveyard.push_back(p);
        if (!p || capturing) return;
        (void)hipDeviceSynchronize();
        (void)hipFree(p);
    }
    // One allocation holding `spans` back to back, copied on the setup stream under RelaxCapture and waited
    // for there. On failure (no stream: hipErrorInvalidValue) nothing stays allocated and *dev is null.
    hipError_t upload(std::initializer_list<HostSpan> spans, void **dev);
private:
    hipStream_t setup = nullptr;
    std::vector<void *> graveyard;
};

// Tables by key in insertion order, 4 of them unless more are pinned; freed with the context, its device current.
template <class Key, class Payload>
class TableCache {
public:
    struct Entry : Payload { Key key{}; void *tab = nullptr; bool pinned = false; };
    ~TableCache() { for (Entry &e : entries) (void)hipFree(e.tab); }
    // The entry of `key`, or null with *rc the error of a failed build. A miss first retires the oldest unpinned
    // entry if 4 are held; then build(Entry &) fills tab and the payload (0, or the error it recorded with nothing
    // left allocated: nothing is inserted). capturing && pin: the entry is never evicted again.
    template <class Build>
    Entry *get(CtxMemory &m, const Key &key, bool capturing, bool pin, int *rc, Build build) {
        auto hit = std::find_if(entries.begin(), entries.end(), [&](const Entry &e) { return e.key == key; });
        if (hit == entries.end()) {
            auto old = std::find_if(entries.begin(), entries.end(), [](const Entry &e) { return !e.pinned; });
            if (entries.size() >= 4 && old != entries.end()) {
                m.retire(old->tab, capturing);
                entries.erase(old);
            }
            Entry e;
            e.key = key;
            if ((*rc = build(e)) != 0) return nullptr;
            hit = entries.insert(entries.end(), std::move(e));
        }
        if (capturing && pin) hit->pinned = true;
        return &*hit;
    }
private:
    std::vector<Entry> entries;
};

}  // namespace bugseg
