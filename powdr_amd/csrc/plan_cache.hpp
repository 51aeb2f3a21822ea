// The cache of plans, written once: small tables derived from a caller's host tables (gather jobs, bus classifications, record
// masks, substitution tables), found again by the CONTENT of those host tables.
//   key        a list of byte ranges. A hit is confirmed by comparing every range, lengths included, against the copy the entry
//              owns; the 64-bit hash only finds the entry and is never trusted. The caller's ranges are read in place: they are
//              copied once, when a plan is inserted.
//   collision  an entry with the same hash and other contents is replaced by the newer one.
//   capacity   at capacity the least recently used entry goes (0: unbounded). Plans are handed out as shared_ptr, so a launch in
//              flight keeps its plan alive while another host thread evicts it.
//   build      runs UNDER THE CACHE'S LOCK, on a miss only: two threads that ask for the same key build once. It may be slow (the
//              device caches allocate and upload in it, hipMalloc included); other keys of the same cache wait for it. A failed
//              build inserts nothing, evicts nothing and returns its code: the victim is chosen after the build has succeeded.
// Host code without HIP in it (tools/plan_cache_selftest_main.cpp compiles it with a plain host compiler). Not part of the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace pw {

// 8 bytes per step (the bytecode of an un-optimised APC is megabytes), the tail byte by byte
inline uint64_t hash_bytes(const void* p, size_t n, uint64_t h) {
    const unsigned char* c = (const unsigned char*)p;
    for (; n >= 8; n -= 8, c += 8) {
        uint64_t w;
        memcpy(&w, c, 8);
        h ^= w; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29;
    }
    for (; n; --n, ++c) { h ^= *c; h *= 1099511628211ull; }
    return h;
}

struct KeyPart { const void* p; size_t bytes; };
template <class T> KeyPart key_part(const T* p, size_t n) { return {p, n * sizeof(T)}; }
template <class T> KeyPart key_part(const std::vector<T>& v) { return {v.data(), v.size() * sizeof(T)}; }
template <class T> KeyPart key_value(const T& v) { return {&v, sizeof(T)}; }  // a plain value without padding bytes

struct KeyHash {
    uint64_t operator()(std::initializer_list<KeyPart> key) const {
        uint64_t h = 1469598103934665603ull;
        for (const KeyPart& k : key) {
            h = hash_bytes(&k.bytes, sizeof k.bytes, h);
            h = hash_bytes(k.p, k.bytes, h);
        }
        return h;
    }
};

// Hash: a parameter so that the self-test can force collisions; the product uses the default everywhere.
template <class Plan, class Hash = KeyHash>
class PlanCache {
public:
    explicit PlanCache(size_t capacity) : capacity_(capacity) {}
    PlanCache(const PlanCache&) = delete;
    PlanCache& operator=(const PlanCache&) = delete;

    // build(Plan&) -> 0 or an error code
    template <class Build>
    int get(std::initializer_list<KeyPart> key, Build build, std::shared_ptr<const Plan>& out) {
        const uint64_t h = Hash()(key);
        std::lock_guard<std::mutex> lk(mu_);
        auto it = entries_.find(h);
        if (it != entries_.end() && same(it->second.key, key)) {
            it->second.last_use = ++clock_;
            out = it->second.plan;
            return 0;
        }
        auto plan = std::make_shared<Plan>();
        if (int rc = build(*plan)) return rc;
        if (it != entries_.end()) {
            entries_.erase(it);  // 64-bit hash collision: the newer tables take the slot
        } else if (capacity_ && entries_.size() >= capacity_) {
            auto victim = entries_.begin();
            for (auto j = entries_.begin(); j != entries_.end(); ++j) if (j->second.last_use < victim->second.last_use) victim = j;
            entries_.erase(victim);
        }
        Entry& e = entries_[h];
        for (const KeyPart& k : key) {
            const unsigned char* len = (const unsigned char*)&k.bytes;
            e.key.insert(e.key.end(), len, len + sizeof k.bytes);
            if (k.bytes) e.key.insert(e.key.end(), (const unsigned char*)k.p, (const unsigned char*)k.p + k.bytes);
        }
        e.plan = std::move(plan);
        e.last_use = ++clock_;
        out = e.plan;
        return 0;
    }

private:
    struct Entry {
        std::vector<unsigned char> key;  // per part: its length (a size_t), then its bytes
        std::shared_ptr<const Plan> plan;
        uint64_t last_use = 0;
    };
    static bool same(const std::vector<unsigned char>& stored, std::initializer_list<KeyPart> key) {
        size_t at = 0;
        for (const KeyPart& k : key) {
            size_t bytes;
            if (stored.size() - at < sizeof bytes) return false;
            memcpy(&bytes, stored.data() + at, sizeof bytes);
            at += sizeof bytes;
            if (bytes != k.bytes || stored.size() - at < bytes) return false;
            if (bytes && memcmp(stored.data() + at, k.p, bytes) != 0) return false;
            at += bytes;
        }
        return at == stored.size();
    }

    const size_t capacity_;
    std::mutex mu_;
    std::unordered_map<uint64_t, Entry> entries_;
    uint64_t clock_ = 0;
};

}  // namespace pw
