// csrc/batch_buffers.hpp as a host program (tests/test_batch_buffers_host.py): the runtime calls the header makes are defined here as
// fakes over malloc that log every call and count what is live, and the scenarios below print what the buffers and the ring hand out.
// The output: "scenario NAME", then a line a runtime call ("sync", "malloc device BYTES", "free pinned", "event_record ID" ...) and
// the scenario's own lines ("state ...", "slot ...", "live ...").
#include "batch_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace {
std::set<void*> g_device, g_pinned, g_events;
long g_allocations = 0, g_fail_at = 0;         // the g_fail_at-th allocation from now on fails (0: none)
int g_event_ids = 0;
void* const kPoison = reinterpret_cast<void*>(0x10);      // what a failed allocation leaves in *ptr

hipError_t fake_allocate(std::set<void*>& live, const char* what, void** ptr, size_t bytes)
{
    ++g_allocations;
    if (g_allocations == g_fail_at) { std::printf("malloc %s %zu failed\n", what, bytes); *ptr = kPoison; return hipErrorOutOfMemory; }
    *ptr = std::malloc(bytes);
    std::memset(*ptr, 0xab, bytes);
    live.insert(*ptr);
    std::printf("malloc %s %zu\n", what, bytes);
    return hipSuccess;
}
hipError_t fake_free(std::set<void*>& live, const char* what, void* ptr)
{
    if (!live.erase(ptr)) { std::printf("free %s of a block that is not live\n", what); std::abort(); }
    std::free(ptr);
    std::printf("free %s\n", what);
    return hipSuccess;
}
int event_id(hipEvent_t e)
{
    if (!g_events.count(e)) { std::printf("use of an event that is not live\n"); std::abort(); }
    return *reinterpret_cast<int*>(e);
}
void fail_next(long n) { g_allocations = 0; g_fail_at = n; }
void live() { std::printf("live device %zu pinned %zu events %zu\n", g_device.size(), g_pinned.size(), g_events.size()); }
template <class B> void state(const B& b) { std::printf("state null %d capacity %zu\n", b.template as<char>() == nullptr ? 1 : 0, b.capacity()); }
bool g_before = false;                         // what *grew holds before a call, in alternation: the call has to write it
template <class B> void grow(B& b, size_t bytes)
{
    bool grew = g_before = !g_before;
    const int failed = b.grow(nullptr, bytes, &grew) != hipSuccess ? 1 : 0;
    std::printf("grow %zu -> %d grew %d\n", bytes, failed, (int)grew);
}
template <class R> void reserve(R& r, size_t slot_bytes)
{
    bool grew = g_before = !g_before;
    const int failed = r.reserve(nullptr, slot_bytes, &grew) != hipSuccess ? 1 : 0;
    std::printf("reserve %zu -> %d grew %d stride %zu count %llu\n", slot_bytes, failed, (int)grew, r.stride(), (unsigned long long)r.count());
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return fake_allocate(g_device, "device", ptr, size); }
hipError_t hipFree(void* ptr) { return fake_free(g_device, "device", ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int flags)
{
    if (flags != hipHostMallocDefault) { std::printf("hipHostMalloc with flags %u\n", flags); std::abort(); }
    return fake_allocate(g_pinned, "pinned", ptr, size);
}
hipError_t hipHostFree(void* ptr) { return fake_free(g_pinned, "pinned", ptr); }
hipError_t hipStreamSynchronize(hipStream_t) { std::printf("sync\n"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags)
{
    if (flags != hipEventDisableTiming) { std::printf("hipEventCreateWithFlags with flags %u\n", flags); std::abort(); }
    *event = reinterpret_cast<hipEvent_t>(new int(g_event_ids));
    g_events.insert(*event);
    std::printf("event_create %d\n", g_event_ids++);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event)
{
    std::printf("event_destroy %d\n", event_id(event));
    g_events.erase(event);
    delete reinterpret_cast<int*>(event);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) { std::printf("event_sync %d\n", event_id(event)); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t event, hipStream_t) { std::printf("event_record %d\n", event_id(event)); return hipSuccess; }
}

namespace {
constexpr int kSlots = 4;

// A buffer grown twice with a grow that fits in between, written over its whole capacity, then destroyed.
template <class B> void buffer_scenario(const char* name)
{
    std::printf("scenario %s\n", name);
    {
        B b;
        state(b);
        grow(b, 0);
        grow(b, 100);
        std::memset(b.template as<char>(), 1, b.capacity());
        state(b);
        grow(b, 100);
        grow(b, 7);
        grow(b, 101);
        std::memset(b.template as<char>(), 2, b.capacity());
        state(b);
        std::printf("release\n");
        b.release();
        state(b);
        grow(b, 5);
        b.template as<double>();                // (the typed accessor is a template over any T)
        std::printf("destroy\n");
    }
    live();
}

// An allocation that fails: the buffer is empty, a later grow serves it and the destructor frees once.
template <class B> void failure_scenario(const char* name)
{
    std::printf("scenario %s\n", name);
    {
        B b;
        grow(b, 64);
        fail_next(1);
        grow(b, 128);
        state(b);
        live();
        grow(b, 32);
        std::memset(b.template as<char>(), 3, b.capacity());
        state(b);
        fail_next(1);
        grow(b, 256);
        std::printf("destroy\n");
    }
    fail_next(0);
    live();
}

void use(SlotRing<kSlots>& r, bool commit = true)
{
    char* slot = nullptr;
    const int rc = (int)r.acquire(slot);
    std::memset(slot, 4, r.stride());           // (the whole slot is the ring's to write)
    std::printf("slot %d count %llu rc %d\n", r.slot_index(), (unsigned long long)r.count(), rc);
    if (commit) std::printf("commit -> %d\n", (int)r.commit(nullptr));
}

// Ten uses; a use without a commit; a reserve that fits; a growth and six more uses; a restart; a second growth; destruction.
void ring_scenario()
{
    std::printf("scenario ring\n");
    {
        SlotRing<kSlots> r;
        reserve(r, 48);
        for (int i = 0; i < 10; ++i) use(r);
        std::printf("uncommitted\n");
        use(r, false);
        use(r, false);
        use(r);
        reserve(r, 48);
        reserve(r, 16);
        reserve(r, 80);
        for (int i = 0; i < 6; ++i) use(r);
        std::printf("restart\n");
        r.restart();
        for (int i = 0; i < 5; ++i) use(r);
        reserve(r, 81);
        use(r);
        std::printf("destroy\n");
    }
    live();
}

// A ring whose block fails to grow: no slot until a later reserve, which serves it; the events are created once.
void ring_failure_scenario()
{
    std::printf("scenario ring_failure\n");
    {
        SlotRing<kSlots> r;
        fail_next(1);
        reserve(r, 32);
        live();
        reserve(r, 32);
        use(r);
        fail_next(1);
        reserve(r, 64);
        reserve(r, 8);
        use(r);
        std::printf("destroy\n");
    }
    fail_next(0);
    live();
}

// A ring never reserved and a buffer never grown are destroyed without a call.
void untouched_scenario()
{
    std::printf("scenario untouched\n");
    { SlotRing<kSlots> r; DeviceBuffer d; PinnedBuffer p; std::printf("destroy\n"); }
    live();
}
}  // namespace

int main()
{
    buffer_scenario<DeviceBuffer>("device");
    buffer_scenario<PinnedBuffer>("pinned");
    failure_scenario<DeviceBuffer>("device_failure");
    failure_scenario<PinnedBuffer>("pinned_failure");
    ring_scenario();
    ring_failure_scenario();
    untouched_scenario();
    return 0;
}
