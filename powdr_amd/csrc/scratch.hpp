// The scratch contract of the device pipelines, written once: a context's buffers are counted, their peak is noted and
// they are released on every path because they are DECLARED as its members, not because a list names them.
//   Scratch        what a context derives from. A buffer registers with it where it is declared (Buf x{*this}); a stage with buffers of
//                  its own (time_index::Stage, register_states::Ctx) is a Scratch constructed with its owner and counts as part of it.
//   Scratch::Buf   released when a call ends and counted (the default), or kStays: kept between calls and counted. A buffer that is
//                  not accounted at all stays a plain DeviceBuf. ensure() raises the peak itself.
//   extra          bytes outside the context that belong to the call: the handle under construction.
//   ScratchCall    the guard of one entry-point call: a fresh peak and fresh statistics, the sticky HIP error cleared, everything
//                  released on every exit; bound() = the caller's scratch bound, or by default half of what the device has room for.
//   with_temp      a rocPRIM call, asked for its temporary storage and then run.
//   Image          a host image of small device tables, uploaded into a Buf in one copy.
// Not part of the C ABI.
#pragma once
#include "bus_shared.hpp"

#include <cstring>
#include <initializer_list>

namespace pw {

class Scratch {
public:
    enum Kind { kReleased, kStays };

    class Buf : public DeviceBuf {
    public:
        explicit Buf(Scratch& owner, Kind kind = kReleased) : owner_(owner), next_(owner.bufs_), stays_(kind == kStays) { owner.bufs_ = this; }
        int ensure(size_t need) {
            const int rc = DeviceBuf::ensure(need);
            owner_.note();
            return rc;
        }

    private:
        friend class Scratch;
        Scratch& owner_;
        Buf* const next_;
        const bool stays_;
    };

    Scratch() = default;
    explicit Scratch(Scratch& owner) : owner_(&owner), next_(owner.stages_) { owner.stages_ = this; }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    virtual ~Scratch() = default;

    // the bytes of the buffers, those of the stages included: what a pipeline reports as its scratch bytes
    size_t held() const {
        size_t s = 0;
        for (const Buf* b = bufs_; b; b = b->next_) s += b->bytes;
        for (const Scratch* c = stages_; c; c = c->next_) s += c->held();
        return s;
    }
    // the most held() + extra since the call began (kept by the outermost owner)
    size_t peak() const { return peak_; }
    void set_extra(size_t bytes) {
        root().extra_ = bytes;
        note();
    }

    // everything but the buffers that stay; a context that has more to drop (the memory tree's kept levels) overrides it
    virtual void release() { release_except({}); }
    void release_except(std::initializer_list<const Buf*> survivors) {
        for (Buf* b = bufs_; b; b = b->next_)
            if (!b->stays_ && std::find(survivors.begin(), survivors.end(), b) == survivors.end()) b->release();
        for (Scratch* c = stages_; c; c = c->next_) c->release_except(survivors);
    }

    // the pipeline's own statistics (they are the context's, not the scratch's): cleared where a call begins
    virtual void reset_stats() {}

private:
    friend class ScratchCall;
    Scratch& root() { return owner_ ? owner_->root() : *this; }
    void note() {
        Scratch& r = root();
        r.peak_ = std::max(r.peak_, r.held() + r.extra_);
    }
    Scratch* const owner_ = nullptr;
    Scratch* const next_ = nullptr;
    Scratch* stages_ = nullptr;
    Buf* bufs_ = nullptr;
    size_t peak_ = 0, extra_ = 0;
};

// One call of an entry point on its context. kContinues: a call on a handle of an earlier call (pw_execution_blocks_count,
// pw_apc_sources_gather), whose peak and statistics stand.
class ScratchCall {
public:
    enum Kind { kFresh, kContinues };
    explicit ScratchCall(Scratch& cx, Kind kind = kFresh) : cx_(cx) {
        if (kind == kFresh) {
            cx.peak_ = 0;
            cx.reset_stats();
        }
        cx.extra_ = 0;
        (void)hipGetLastError();
    }
    // ... of an entry point that answers with a handle, a status and its info
    template <class Handle>
    ScratchCall(Scratch& cx, Handle** out, uint32_t* status, uint64_t* info) : ScratchCall(cx) {
        *out = nullptr;
        *status = 0;
        *info = 0;
    }
    ~ScratchCall() {
        cx_.release();
        cx_.extra_ = 0;
    }
    ScratchCall(const ScratchCall&) = delete;
    ScratchCall& operator=(const ScratchCall&) = delete;
    size_t bound(size_t scratch_bytes) const { return scratch_bytes ? scratch_bytes : bus::default_bound(cx_.held()); }

private:
    Scratch& cx_;
};

// a rocPRIM call f(temporary storage, its size): asked for the size, then run in `temp`
template <class F>
inline int with_temp(Scratch::Buf& temp, F f) {
    size_t bytes = 0;
    PW_HIP_TRY(f(nullptr, bytes));
    PW_TRY(temp.ensure(std::max<size_t>(bytes, 16)));
    PW_HIP_TRY(f(temp.p, bytes));
    return 0;
}

// a host image of device tables, every piece 16-byte aligned
struct Image {
    std::vector<char> bytes;
    template <class T>
    size_t put(const std::vector<T>& v) {
        const size_t at = (bytes.size() + 15) & ~(size_t)15;
        bytes.resize(at + v.size() * sizeof(T));
        if (!v.empty()) memcpy(bytes.data() + at, v.data(), v.size() * sizeof(T));
        return at;
    }
    int upload(Scratch::Buf& b, hipStream_t st) {
        bytes.resize(bytes.size() + 16);
        PW_TRY(b.ensure(bytes.size()));
        PW_HIP_TRY(hipMemcpyAsync(b.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
        return 0;
    }
};

}  // namespace pw
