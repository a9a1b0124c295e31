// The buffers a batch's state owns (BatchState in cpprob_hip.hip): a device or pinned block that is freed with its owner and replaced
// only through grow(), which waits for the stream first -- copies and kernels enqueued earlier may still read the block it frees --, and
// the ring of pinned slots a call writes its descriptors into while the copies of the calls before it are still in flight.  Host code
// over the HIP runtime's C API alone, without the context: the functions return hipError_t and the callers turn an error into their own;
// tests/test_batch_buffers_host.py builds the header as a host program against fakes of the runtime calls it makes.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

struct BatchDeviceMemory {
    static hipError_t allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct BatchPinnedMemory {
    static hipError_t allocate(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};

// One block and its capacity in bytes; null and 0 before the first growth, after release() and after an allocation that failed.
template <class Memory>
class BatchBuffer {
public:
    BatchBuffer() = default;
    BatchBuffer(const BatchBuffer&) = delete;
    BatchBuffer& operator=(const BatchBuffer&) = delete;
    ~BatchBuffer() { release(); }

    template <class T> T* as() const { return static_cast<T*>(p_); }
    size_t capacity() const { return bytes_; }

    void release()
    {
        if (p_) Memory::free(p_);
        p_ = nullptr; bytes_ = 0;
    }

    // Room for bytes: nothing where they fit; else the stream is waited for, the block freed and a new one allocated (its contents
    // are not kept).  grew: whether the block was freed -- what the caller keeps about its contents is void then, also where the
    // allocation fails.
    hipError_t grow(hipStream_t stream, size_t bytes, bool* grew = nullptr)
    {
        if (grew) *grew = false;
        if (bytes <= bytes_) return hipSuccess;
        if (hipError_t e = hipStreamSynchronize(stream)) return e;
        release();
        if (grew) *grew = true;
        if (hipError_t e = Memory::allocate(&p_, bytes)) { p_ = nullptr; return e; }
        bytes_ = bytes;
        return hipSuccess;
    }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};
using DeviceBuffer = BatchBuffer<BatchDeviceMemory>;
using PinnedBuffer = BatchBuffer<BatchPinnedMemory>;

// kSlots pinned slots written in turn, an event a slot: use i writes slot i % kSlots, once the copies that read it kSlots uses ago have
// run.  A use is acquire() -- wait for the slot, get its address --, the caller's writes and copies, commit() -- record the slot's
// event behind them, move on; an acquire() without a commit() hands out the same slot again.
template <int kSlots>
class SlotRing {
public:
    SlotRing() = default;
    SlotRing(const SlotRing&) = delete;
    SlotRing& operator=(const SlotRing&) = delete;
    ~SlotRing() { for (hipEvent_t e : done_) if (e) (void)hipEventDestroy(e); }

    // Slots of slot_bytes: where that exceeds the stride the block is grown (PinnedBuffer::grow: the stream is waited for), the
    // stride is slot_bytes from then on and the count starts at 0 again; the events are created once.
    hipError_t reserve(hipStream_t stream, size_t slot_bytes, bool* grew = nullptr)
    {
        if (grew) *grew = false;
        if (slot_bytes > stride_) {
            stride_ = 0; count_ = 0;
            if (hipError_t e = pin_.grow(stream, (size_t)kSlots * slot_bytes, grew)) return e;
            stride_ = slot_bytes;
        }
        for (hipEvent_t& e : done_) if (!e) if (hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming)) { e = nullptr; return err; }
        return hipSuccess;
    }
    hipError_t acquire(char*& slot)
    {
        slot = pin_.template as<char>() + (size_t)slot_index() * stride_;
        return count_ >= (uint64_t)kSlots ? hipEventSynchronize(done_[slot_index()]) : hipSuccess;
    }
    hipError_t commit(hipStream_t stream)
    {
        if (hipError_t e = hipEventRecord(done_[slot_index()], stream)) return e;
        ++count_;
        return hipSuccess;
    }
    void restart() { count_ = 0; }             // (the caller has drained the stream: no slot is being read)
    uint64_t count() const { return count_; }
    int slot_index() const { return (int)(count_ % (uint64_t)kSlots); }
    size_t stride() const { return stride_; }

private:
    PinnedBuffer pin_;
    hipEvent_t done_[kSlots] = {};
    size_t stride_ = 0;
    uint64_t count_ = 0;
};
