// Stand-alone self-test of powdr_amd/csrc/plan_cache.hpp (header-only host code): built with UBSan + ASan, and with TSan where
// the compiler has it, and run as a child process by tests/test_plan_cache.py.
//   plan_cache_selftest            every case
//   plan_cache_selftest threads    only the threaded case (the TSan build)
#include "../powdr_amd/csrc/plan_cache.hpp"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

namespace {

std::atomic<int> g_built{0}, g_destroyed{0};
struct FakePlan {
    int id = 0;
    FakePlan() = default;
    FakePlan(const FakePlan&) = delete;
    FakePlan& operator=(const FakePlan&) = delete;
    ~FakePlan() { ++g_destroyed; }
};
using Ptr = std::shared_ptr<const FakePlan>;

struct ConstantHash { uint64_t operator()(std::initializer_list<pw::KeyPart>) const { return 7; } };

int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("  FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } } while (0)

// get() of the key (a, b) with a build that counts and names the plan `id`
template <class Cache>
int get2(Cache& c, const std::string& a, const std::string& b, int id, Ptr& out, int fail_with = 0) {
    return c.get({pw::key_part(a.data(), a.size()), pw::key_part(b.data(), b.size())}, [&](FakePlan& p) {
        if (fail_with) return fail_with;
        ++g_built;
        p.id = id;
        return 0;
    }, out);
}
template <class Cache>
Ptr get1(Cache& c, int k) {
    Ptr out;
    const int rc = c.get({pw::key_value(k)}, [&](FakePlan& p) { ++g_built; p.id = k; return 0; }, out);
    CHECK(rc == 0 && out && out->id == k);
    return out;
}

void case_hit() {
    pw::PlanCache<FakePlan> c(4);
    Ptr a, b;
    const int built = g_built;
    CHECK(get2(c, "abc", "", 1, a) == 0 && g_built == built + 1);
    CHECK(get2(c, "abc", "", 2, b) == 0 && g_built == built + 1);
    CHECK(a && a.get() == b.get() && a->id == 1);
}

void case_part_lengths() {
    pw::PlanCache<FakePlan> c(4);
    Ptr a, b, a2;
    const int built = g_built;
    CHECK(get2(c, "ab", "c", 1, a) == 0);
    CHECK(get2(c, "a", "bc", 2, b) == 0);
    CHECK(g_built == built + 2 && a.get() != b.get() && a->id == 1 && b->id == 2);
    CHECK(get2(c, "ab", "c", 3, a2) == 0 && a2.get() == a.get() && g_built == built + 2);
    // the same under one hash: lengths are compared, not only hashed
    pw::PlanCache<FakePlan, ConstantHash> d(4);
    Ptr e, f;
    CHECK(get2(d, "ab", "c", 4, e) == 0 && get2(d, "a", "bc", 5, f) == 0 && e.get() != f.get() && f->id == 5);
    // a key that is a prefix of the stored one, and one with a part less
    Ptr g, h;
    CHECK(get2(d, "a", "b", 6, g) == 0 && g->id == 6);
    CHECK(d.get({pw::key_part("a", 1)}, [&](FakePlan& p) { p.id = 7; return 0; }, h) == 0 && h->id == 7);
}

void case_collision_replaces() {
    pw::PlanCache<FakePlan, ConstantHash> c(4);
    Ptr a, b, a2;
    const int built = g_built;
    CHECK(get2(c, "first", "", 1, a) == 0);
    CHECK(get2(c, "second", "", 2, b) == 0 && b->id == 2);
    CHECK(get2(c, "second", "", 9, b) == 0 && b->id == 2 && g_built == built + 2);  // the newer one holds the slot
    CHECK(get2(c, "first", "", 3, a2) == 0 && a2->id == 3 && g_built == built + 3);  // the first builds again
    CHECK(a->id == 1);  // and the replaced plan lives while it is held
}

void case_lru() {
    const int cap = 3;
    pw::PlanCache<FakePlan> c(cap);
    const int built = g_built;
    for (int k = 0; k < cap; ++k) get1(c, k);
    get1(c, 0);    // a hit: key 1 is now the least recently used
    get1(c, cap);  // evicts exactly key 1
    CHECK(g_built == built + cap + 1);
    get1(c, 0); get1(c, 2); get1(c, cap);
    CHECK(g_built == built + cap + 1);  // all three still there
    get1(c, 1);
    CHECK(g_built == built + cap + 2);  // key 1 was gone
}

void case_held_plan_outlives_eviction() {
    pw::PlanCache<FakePlan> c(1);
    Ptr held = get1(c, 1);
    const int destroyed = g_destroyed;
    get1(c, 2);  // evicts key 1 (the temporary for key 2 dies with the cache)
    CHECK(g_destroyed == destroyed && held->id == 1);
    held.reset();
    CHECK(g_destroyed == destroyed + 1);
}

void case_failed_build() {
    pw::PlanCache<FakePlan> c(2);
    get1(c, 1); get1(c, 2);
    const int built = g_built, destroyed = g_destroyed;
    Ptr out;
    CHECK(get2(c, "x", "y", 3, out, 42) == 42 && !out);
    CHECK(g_destroyed == destroyed + 1);  // only the plan that failed to build
    get1(c, 1); get1(c, 2);
    CHECK(g_built == built);  // nothing was evicted at capacity
    CHECK(get2(c, "x", "y", 3, out) == 0 && out->id == 3 && g_built == built + 1);  // and nothing was inserted
    // under one hash: a failed build leaves the entry it would have replaced
    pw::PlanCache<FakePlan, ConstantHash> d(2);
    Ptr a, b;
    CHECK(get2(d, "first", "", 1, a) == 0 && get2(d, "second", "", 2, b, 5) == 5);
    const int built2 = g_built;
    CHECK(get2(d, "first", "", 1, b) == 0 && b.get() == a.get() && g_built == built2);
}

void case_unbounded() {
    pw::PlanCache<FakePlan> c(0);
    const int built = g_built, destroyed = g_destroyed;
    for (int k = 0; k < 500; ++k) get1(c, k);
    for (int k = 0; k < 500; ++k) get1(c, k);
    CHECK(g_built == built + 500 && g_destroyed == destroyed);
}

void case_threads() {
    pw::PlanCache<FakePlan> c(8);
    std::atomic<int> built{0}, wrong{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < 8; ++t)
        ts.emplace_back([&, t] {
            for (int i = 0; i < 1000; ++i) {
                const int k = (i + t) % 4;
                Ptr out;
                const int rc = c.get({pw::key_value(k)}, [&](FakePlan& p) { ++built; p.id = k; return 0; }, out);
                if (rc || !out || out->id != k) ++wrong;
            }
        });
    for (auto& t : ts) t.join();
    CHECK(built == 4 && wrong == 0);
}

void case_hash() {
    const char s[] = "0123456789abcdef0123";
    // an unaligned start gives the same value as an aligned copy, and every byte of the tail counts
    char shifted[32];
    memcpy(shifted + 1, s, 20);
    CHECK(pw::hash_bytes(s, 20, 1) == pw::hash_bytes(shifted + 1, 20, 1));
    CHECK(pw::hash_bytes(s, 20, 1) != pw::hash_bytes(s, 19, 1) && pw::hash_bytes(s, 16, 1) != pw::hash_bytes(s, 17, 1));
    CHECK(pw::hash_bytes(nullptr, 0, 5) == 5);
}

}  // namespace

int main(int argc, char** argv) {
    const bool only_threads = argc > 1 && strcmp(argv[1], "threads") == 0;
    struct { const char* name; void (*run)(); bool threaded; } cases[] = {
        {"hit", case_hit, false}, {"part lengths", case_part_lengths, false}, {"collision replaces", case_collision_replaces, false},
        {"least recently used", case_lru, false}, {"held plan outlives eviction", case_held_plan_outlives_eviction, false},
        {"failed build", case_failed_build, false}, {"unbounded", case_unbounded, false}, {"hash", case_hash, false},
        {"threads", case_threads, true},
    };
    for (auto& c : cases) {
        if (only_threads && !c.threaded) continue;
        const int before = g_failures;
        c.run();
        printf("%s: %s\n", c.name, g_failures == before ? "ok" : "FAILED");
    }
    return g_failures ? 1 : 0;
}
