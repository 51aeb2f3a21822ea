// Selecting APC calls on the device (include/powdr_prover.h pw_apc_calls_from_states): from the states of an execution
// — pcs and register values in time order — and the chosen APCs with their optimistic constraints, the non-overlapping calls the
// reference's ApcCandidates (autoprecompiles/src/execution/candidates.rs) extracts while the execution runs, and per APC what became
// of every pc match.
//   candidates  apc_calls_match_kernel    one lane per position looks its pc up in the sorted distinct start pcs and counts the APCs
//                                         that start there; an exclusive scan places them; apc_calls_emit_kernel writes the candidates
//                                         position-major, apc_id ascending, as (position << 32 | apc)
//   validity    apc_calls_eval_kernel     one lane per (candidate, chunk of kChunk constraints): an APC with thousands of constraints
//                                         is thousands of work items next to its neighbour's one, never one long lane. A false
//                                         constraint lowers fail[candidate] to its step (atomicMin); apc_calls_classify_kernel turns
//                                         that, the cycle count and the end of the execution into refused / failed / aborted / done
//   components  the done candidates compacted in order; an inclusive max-scan of their ends: a candidate that starts at or after
//               every earlier end starts a component — no candidate of one component overlaps one of another
//   fold        apc_calls_fold_kernel     one lane per component: a component of one is a call; up to the threshold the lane runs the
//                                         reference's pair loop on its component; a longer one is listed for
//               apc_calls_fold_long_kernel  one wave per long component: (start, end, rank, discarded) of kStage candidates staged in
//                                         LDS, the live candidate i meets the 64 candidates behind it per step (a ballot finds the
//                                         first that outranks it; everything live before that is discarded), candidates beyond the
//                                         staged stretch are read and marked in global memory
//   read-out    apc_calls_tally_kernel    discarded / call per APC; the survivors compacted into the call list
// Counters are added once per distinct key of a wave (a hot APC is one address, not one atomic per lane).
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "register_states.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

#include <map>
#include <memory>

namespace pw {

namespace {

using namespace bus;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kChunk = 32;          // constraints per work item
constexpr u64 kLongDefault = 32;         // components of more candidates take the long path
constexpr uint32_t kStage = 2048;        // candidates the long path stages in LDS at a time
constexpr int kCounters = 7;             // per APC: matches, refused, failed, aborted, done, discarded, calls
enum { kMatches = 0, kRefused, kFailed, kAborted, kDone, kDiscarded, kCalls };

struct ApcDev { u64 first, n; uint32_t cycle, rank, chunks, pad; };        // rank: dense over (priority, cycle_count), higher wins
struct OpDev { uint32_t kind, idx, reg, shift; u64 value; };
struct ConDev { OpDev l, r; };
// the state table and the APC tables as the kernels read them
struct Tables {
    const uint32_t* pcs;
    const uint32_t* regs;
    u64 n_states;
    uint32_t limb_mask;
    const ApcDev* apcs;
    const ConDev* cons;
    const uint32_t *slot_pcs, *slot_first, *slot_apcs;  // the distinct start pcs ascending; slot s holds slot_apcs[slot_first[s] .. slot_first[s + 1])
    uint32_t n_slots;
};

struct ChunksOf {
    const ApcDev* apcs;
    __device__ u64 operator()(u64 cand) const { return apcs[(uint32_t)cand].chunks; }
};

__device__ __forceinline__ uint32_t find_slot_of(const Tables& t, uint32_t pc) {
    uint32_t lo = 0, hi = t.n_slots;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.slot_pcs[mid] < pc) lo = mid + 1;
        else hi = mid;
    }
    return lo < t.n_slots && t.slot_pcs[lo] == pc ? lo : kNone;
}

// counters[key] += the lanes of the wave that hold key (kEmpty: none): one atomic per distinct key. Every lane of the wave calls.
__device__ __forceinline__ void wave_count(u64* __restrict__ counters, u64 key) {
    u64 todo = __builtin_amdgcn_ballot_w64(key != kEmpty);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const u64 k = __shfl(key, leader, 64);
        const u64 same = __builtin_amdgcn_ballot_w64(key == k);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(counters + k, (u64)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kBlock) void apc_calls_match_kernel(Tables t, uint32_t* __restrict__ count, u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    uint32_t s = kNone;
    if (i < t.n_states) {
        s = find_slot_of(t, t.pcs[i]);
        count[i] = s == kNone ? 0u : t.slot_first[s + 1] - t.slot_first[s];
    }
    u64 todo = __builtin_amdgcn_ballot_w64(s != kNone);
    while (todo) {  // every APC of a slot matches once per lane that holds the slot
        const int leader = __builtin_ctzll(todo);
        const uint32_t k = __shfl(s, leader, 64);
        const u64 same = __builtin_amdgcn_ballot_w64(s == k);
        if ((int)(threadIdx.x & 63u) == leader)
            for (uint32_t a = t.slot_first[k]; a < t.slot_first[k + 1]; ++a) atomicAdd(counters + (u64)t.slot_apcs[a] * kCounters + kMatches, (u64)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kBlock) void apc_calls_emit_kernel(Tables t, const uint32_t* __restrict__ off, u64* __restrict__ cand) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.n_states) return;
    const uint32_t s = find_slot_of(t, t.pcs[i]);
    if (s == kNone) return;
    const uint32_t first = t.slot_first[s], n = t.slot_first[s + 1] - first;
    for (uint32_t k = 0; k < n; ++k) cand[(u64)off[i] + k] = (i << 32) | t.slot_apcs[first + k];  // (below the candidates counted: off is their scan)
}

__device__ __forceinline__ u64 operand(const Tables& t, const OpDev& o, u64 s) {
    if (o.kind == 0u) return o.value;
    if (o.kind == 1u) return t.pcs[s + o.idx];
    return (t.regs[(u64)o.reg * t.n_states + s + o.idx] >> o.shift) & t.limb_mask;
}

// item = base + lane: chunk (item - item_off[c]) of candidate c's constraints. A constraint is checked at step = its largest instr_idx
// if that step is reached: step <= cycle_count and state s + step exists — so every state read lies inside the table.
__global__ __launch_bounds__(kBlock) void apc_calls_eval_kernel(Tables t, const u64* __restrict__ cand, const u64* __restrict__ item_off, u64 n_cand, u64 base, u64 n_items,
                                                                 uint32_t* __restrict__ fail) {
    const u64 item = base + (u64)blockIdx.x * kBlock + threadIdx.x;
    if (item >= n_items) return;
    u64 lo = 0, hi = n_cand;  // the last candidate with item_off <= item
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (item_off[mid] <= item) lo = mid + 1;
        else hi = mid;
    }
    const u64 c = lo - 1, v = cand[c], s = v >> 32;
    const ApcDev a = t.apcs[(uint32_t)v];
    const u64 left = t.n_states - 1 - s, limit = a.cycle < left ? a.cycle : left;
    const u64 k0 = (item - item_off[c]) * kChunk, k1 = k0 + kChunk < a.n ? k0 + kChunk : a.n;
    uint32_t worst = kNone;
    for (u64 k = k0; k < k1; ++k) {
        const ConDev q = t.cons[a.first + k];
        const uint32_t sl = q.l.kind ? q.l.idx : 0u, sr = q.r.kind ? q.r.idx : 0u, step = sl > sr ? sl : sr;
        if (step > limit || step >= worst) continue;
        if (operand(t, q.l, s) != operand(t, q.r, s)) worst = step;
    }
    if (worst != kNone) atomicMin(fail + c, worst);
}

__global__ __launch_bounds__(kBlock) void apc_calls_classify_kernel(Tables t, const u64* __restrict__ cand, const uint32_t* __restrict__ fail, u64 n_cand,
                                                                     uint8_t* __restrict__ done, u64* __restrict__ counters) {
    const u64 c = (u64)blockIdx.x * kBlock + threadIdx.x;
    u64 key = kEmpty;
    if (c < n_cand) {
        const u64 v = cand[c], s = v >> 32;
        const uint32_t f = fail[c], cycle = t.apcs[(uint32_t)v].cycle;
        const int cls = f == 0u ? kRefused : f != kNone ? kFailed : s + cycle > t.n_states - 1 ? kAborted : kDone;
        done[c] = cls == kDone;
        key = (v & 0xffffffffull) * kCounters + cls;
    }
    wave_count(counters, key);
}

__global__ __launch_bounds__(kBlock) void apc_calls_ends_kernel(const u64* __restrict__ V, const ApcDev* __restrict__ apcs, u64 n, uint32_t* __restrict__ end) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) end[i] = (uint32_t)(V[i] >> 32) + apcs[(uint32_t)V[i]].cycle;  // (a done candidate ends inside the table: below 2^32)
}

// mx = the running maximum of the ends: candidate i starts a component iff it starts at or after every earlier end
__global__ __launch_bounds__(kBlock) void apc_calls_cut_kernel(const u64* __restrict__ V, const uint32_t* __restrict__ mx, u64 n, uint8_t* __restrict__ cflag) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) cflag[i] = !i || (uint32_t)(V[i] >> 32) >= mx[i - 1];
}

// counters: [0] the longest component | [1] components listed for the long path
__global__ __launch_bounds__(kBlock) void apc_calls_fold_kernel(const u64* __restrict__ V, const ApcDev* __restrict__ apcs, const uint32_t* __restrict__ cfirst, u64 n_comp,
                                                                 u64 threshold, uint8_t* __restrict__ disc, uint32_t* __restrict__ longs, u64 longs_cap,
                                                                 u64* __restrict__ counters) {
    const u64 c = (u64)blockIdx.x * kBlock + threadIdx.x;
    u64 n = 0;
    if (c < n_comp) {
        const u64 c0 = cfirst[c];
        n = cfirst[c + 1] - c0;
        if (n > threshold) {
            const u64 at = atomicAdd(counters + 1, 1ull);
            if (at < longs_cap) longs[at] = (uint32_t)c;  // (the list holds every component that can be this long)
        } else if (n > 1) {
            // the reference's pair loop: all (i < j) in order; the candidates are in start order, so j overlaps i iff it starts before
            // i's end, and no later j does once one does not
            for (u64 i = 0; i < n; ++i) {
                if (disc[c0 + i]) continue;
                const u64 vi = V[c0 + i];
                const ApcDev ai = apcs[(uint32_t)vi];
                const u64 end_i = (vi >> 32) + ai.cycle;
                for (u64 j = i + 1; j < n; ++j) {
                    const u64 vj = V[c0 + j];
                    if ((vj >> 32) >= end_i) break;
                    if (disc[c0 + j]) continue;
                    if (apcs[(uint32_t)vj].rank > ai.rank) {  // (equal ranks: the earlier insertion wins)
                        disc[c0 + i] = 1;
                        break;
                    }
                    disc[c0 + j] = 1;
                }
            }
        }
    }
    n = ~wave_min(~n);
    if ((threadIdx.x & 63u) == 0u && n > 1) atomicMax(counters, n);
}

// One wave per listed component V[c0 .. c0 + n). The walk is sequential in i; what is parallel is the stretch behind i: lane l holds
// candidate i + 1 + l (then + 64 ...), in range while it starts before i's end. The first live one in range that outranks i discards
// i; every live one in range before it is discarded by i. The same lanes say which candidate is the next live i and hand over its
// end and rank, so a step is one LDS read of 16 bytes per lane, three ballots and the marks.
struct Staged { uint32_t start, end, rank, gone; };
__global__ __launch_bounds__(64) void apc_calls_fold_long_kernel(const u64* __restrict__ V, const ApcDev* __restrict__ apcs, const uint32_t* __restrict__ cfirst,
                                                                  const uint32_t* __restrict__ longs, uint8_t* __restrict__ disc) {
    __shared__ Staged stage[kStage];
    const uint32_t c = longs[blockIdx.x], lane = threadIdx.x;
    const u64 c0 = cfirst[c], n = cfirst[c + 1] - c0;
    for (u64 base = 0; base < n; base += kStage) {
        const uint32_t m = n - base < kStage ? (uint32_t)(n - base) : kStage;
        for (uint32_t k = lane; k < m; k += 64u) {
            const u64 v = V[c0 + base + k];
            const ApcDev a = apcs[(uint32_t)v];
            // (gone: marked from an earlier stretch, or 0)
            stage[k] = Staged{(uint32_t)(v >> 32), (uint32_t)(v >> 32) + a.cycle, a.rank, __atomic_load_n(disc + c0 + base + k, __ATOMIC_RELAXED)};
        }
        __syncthreads();
        uint32_t i = 0, end_i = 0, rank_i = 0;
        bool have = false;  // i is live and end_i, rank_i are its own (everything that steers the loops is uniform over the wave)
        for (;;) {
            if (!have) {  // the next live candidate at or after i
                if (i >= m) break;
                const u64 live = __builtin_amdgcn_ballot_w64(i + lane < m && !stage[i + lane < m ? i + lane : 0].gone);
                if (!live) {
                    i += 64u;
                    continue;
                }
                i += (uint32_t)__builtin_ctzll(live);
                end_i = stage[i].end;
                rank_i = stage[i].rank;
            }
            have = false;
            uint32_t next_i = i + 1u;
            for (u64 j0 = base + i + 1; j0 < n; j0 += 64) {
                const u64 j = j0 + lane;
                const bool staged = j < n && j - base < kStage;
                Staged e{0u, 0u, 0u, 1u};
                bool in_range = false;
                if (staged) {
                    e = stage[j - base];
                    in_range = e.start < end_i;
                } else if (j < n) {
                    const u64 v = V[c0 + j];
                    in_range = (uint32_t)(v >> 32) < end_i;
                    if (in_range) {
                        e.gone = __atomic_load_n(disc + c0 + j, __ATOMIC_RELAXED);
                        e.rank = apcs[(uint32_t)v].rank;
                    }
                }
                const bool meets = in_range && !e.gone;
                const u64 killers = __builtin_amdgcn_ballot_w64(meets && e.rank > rank_i);
                const uint32_t first = killers ? (uint32_t)__builtin_ctzll(killers) : 64u;
                const bool marked = meets && lane < first;
                if (marked) {
                    if (staged) stage[j - base].gone = 1u;
                    else __atomic_store_n(disc + c0 + j, (uint8_t)1, __ATOMIC_RELAXED);
                }
                if (killers && lane == 0u) stage[i].gone = 1u;
                // the first staged candidate of these 64 that is still live is the next i (earlier windows held none: the walk only
                // goes on past a window whose live candidates were all marked)
                const u64 alive = __builtin_amdgcn_ballot_w64(staged && !e.gone && !marked);
                const bool all_in_range = __builtin_amdgcn_ballot_w64(in_range) == ~0ull;
                if (alive) {
                    const int d = __builtin_ctzll(alive);
                    have = true;
                    next_i = (uint32_t)(j0 - base) + (uint32_t)d;
                    end_i = (uint32_t)__builtin_amdgcn_readlane((int)e.end, d);
                    rank_i = (uint32_t)__builtin_amdgcn_readlane((int)e.rank, d);
                }
                __syncthreads();
                if (alive || killers || !all_in_range) break;
            }
            i = next_i;
        }
        __syncthreads();
        for (uint32_t k = lane; k < m; k += 64u) disc[c0 + base + k] = (uint8_t)stage[k].gone;
        __threadfence();  // the marks beyond the stretch are read back by other lanes when it is staged
    }
}

__global__ __launch_bounds__(kBlock) void apc_calls_tally_kernel(const u64* __restrict__ V, const uint8_t* __restrict__ disc, u64 n, uint8_t* __restrict__ keep,
                                                                  u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    u64 key = kEmpty;
    if (i < n) {
        keep[i] = !disc[i];
        key = (V[i] & 0xffffffffull) * kCounters + (disc[i] ? kDiscarded : kCalls);
    }
    wave_count(counters, key);
}

struct AcCtx : Scratch {
    Buf small{*this}, count{*this}, off{*this}, cand{*this}, item_off{*this}, fail{*this}, done{*this}, V{*this}, end{*this}, mx{*this}, cflag{*this}, cfirst{*this},
        longs{*this}, disc{*this}, keep{*this}, calls{*this}, temp{*this}, states{*this}, regtab{*this}, tkeys{*this};
    time_index::Stage index{*this};      // of the trace route
    register_states::Ctx stage{*this};  // of the trace route with registers (register_states.hpp)
    uint64_t long_threshold = 0;  // 0: kLongDefault
    uint64_t stat_candidates = 0, stat_valid = 0, stat_components = 0, stat_longest = 0, stat_long = 0;
    void reset_stats() override { stat_candidates = stat_valid = stat_components = stat_longest = stat_long = 0; }
};
thread_local AcCtx g_ac;

// what the argument check leaves for the device: the tables in the kernels' layout
struct HostTables {
    std::vector<ApcDev> apcs;
    std::vector<ConDev> cons;
    std::vector<uint32_t> slot_pcs, slot_first, slot_apcs;
    u64 max_share = 0;  // the most APCs that start at one pc
    size_t bytes() const { return 256 + apcs.size() * (sizeof(ApcDev) + kCounters * 8 + 4) + cons.size() * sizeof(ConDev) + (slot_pcs.size() * 2 + 1) * 4 + 5 * 16; }
};

// false = -1: cycle_count == 0, a constraint span outside the array, an unknown operand kind, reg >= n_regs, limb * limb_bits >= 32
bool check_tables(const PwApc* apcs, size_t n_apcs, const PwApcConstraint* cons, size_t n_cons, uint32_t n_regs, uint32_t limb_bits, HostTables& h) {
    if ((!apcs && n_apcs) || (!cons && n_cons) || limb_bits < 1u || limb_bits > 32u || n_apcs >= ((size_t)1 << 31)) return false;
    h.cons.resize(n_cons);
    for (size_t k = 0; k < n_cons; ++k) {
        const PwApcOperand* src[2] = {&cons[k].left, &cons[k].right};
        OpDev* dst[2] = {&h.cons[k].l, &h.cons[k].r};
        for (int e = 0; e < 2; ++e) {
            const PwApcOperand& o = *src[e];
            if (o.kind > 2u) return false;
            if (o.kind == 2u && (o.reg >= n_regs || (u64)o.limb * limb_bits >= 32)) return false;
            *dst[e] = OpDev{o.kind, o.kind ? o.instr_idx : 0u, o.kind == 2u ? o.reg : 0u, o.kind == 2u ? o.limb * limb_bits : 0u, o.kind ? 0ull : o.value};
        }
    }
    std::map<std::pair<uint64_t, uint32_t>, uint32_t> ranks;
    std::map<uint32_t, std::vector<uint32_t>> by_pc;
    for (size_t a = 0; a < n_apcs; ++a) {
        if (!apcs[a].cycle_count || apcs[a].first_constraint > n_cons || apcs[a].n_constraints > n_cons - apcs[a].first_constraint) return false;
        ranks[{apcs[a].priority, apcs[a].cycle_count}] = 0;
        by_pc[apcs[a].start_pc].push_back((uint32_t)a);
    }
    uint32_t r = 0;
    for (auto& kv : ranks) kv.second = r++;
    h.apcs.resize(n_apcs);
    for (size_t a = 0; a < n_apcs; ++a)
        h.apcs[a] = ApcDev{apcs[a].first_constraint, apcs[a].n_constraints, apcs[a].cycle_count, ranks[{apcs[a].priority, apcs[a].cycle_count}],
                           (uint32_t)std::min<u64>((apcs[a].n_constraints + kChunk - 1) / kChunk, 0xffffffffu), 0u};
    h.slot_first.push_back(0);
    for (const auto& kv : by_pc) {
        h.slot_pcs.push_back(kv.first);
        h.slot_apcs.insert(h.slot_apcs.end(), kv.second.begin(), kv.second.end());
        h.slot_first.push_back((uint32_t)h.slot_apcs.size());
        h.max_share = std::max<u64>(h.max_share, kv.second.size());
    }
    return true;
}

// Bytes that always suffice for n_states states, before one is read: every position holds at most max_share candidates. 8 per
// position (count, offset); per candidate 29 while it is evaluated (candidate, item offset, fail, done, the compacted copy) and at
// most 24 afterwards (the done ones, then ends, running maximum, flags and component starts, then discards, the list of long
// components, keep flags and the calls); the rest is the temporary storage of the scans and compactions.
size_t calls_need(u64 n_states, u64 cand_max, size_t tables) { return ((size_t)1 << 20) + tables + (size_t)n_states * 9 + (size_t)cand_max * 40; }

}  // namespace

}  // namespace pw

using namespace pw;

struct PwApcCalls {
    std::vector<uint32_t> ids;
    std::vector<uint64_t> from, to, counters, time_keys;
    uint64_t covered = 0, n_states = 0, n_apcs = 0;
};

extern "C" void pw_apc_calls_set_long_threshold(uint64_t n) { g_ac.long_threshold = n; }

extern "C" void pw_apc_calls_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_ac.stat_candidates;
    out[1] = g_ac.stat_valid;
    out[2] = g_ac.stat_components;
    out[3] = g_ac.stat_longest;
    out[4] = g_ac.stat_long;
    out[5] = g_ac.peak();
    out[6] = g_ac.held();
}

extern "C" void pw_apc_calls_destroy(PwApcCalls* e) { delete e; }

extern "C" void pw_apc_calls_sizes(const PwApcCalls* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->ids.size();
    sizes[1] = e->n_apcs;
    sizes[2] = e->covered;
    sizes[3] = e->n_states;
    sizes[4] = e->time_keys.size();
}

extern "C" void pw_apc_calls_read_calls(const PwApcCalls* e, uint32_t* apc_ids, uint64_t* from, uint64_t* to) {
    if (!e) return;
    if (apc_ids) std::copy(e->ids.begin(), e->ids.end(), apc_ids);
    if (from) std::copy(e->from.begin(), e->from.end(), from);
    if (to) std::copy(e->to.begin(), e->to.end(), to);
}

extern "C" void pw_apc_calls_read_counters(const PwApcCalls* e, uint64_t* counters) {
    if (e && counters) std::copy(e->counters.begin(), e->counters.end(), counters);
}

extern "C" void pw_apc_calls_read_time_keys(const PwApcCalls* e, uint64_t* keys) {
    if (e && keys) std::copy(e->time_keys.begin(), e->time_keys.end(), keys);
}

namespace {

std::unique_ptr<PwApcCalls> empty_result(size_t n_apcs, u64 n_states) {
    auto result = std::make_unique<PwApcCalls>();
    result->n_apcs = n_apcs;
    result->n_states = n_states;
    result->counters.assign(n_apcs * kCounters, 0);
    return result;
}

// Everything behind the states: d_pcs[0 .. n_states), n_states > 0, d_regs column-major. `extra` = scratch bytes the caller holds
// through the call. The caller releases cx's buffers.
int select_calls(AcCtx& cx, const uint32_t* d_pcs, const uint32_t* d_regs, u64 n_states, uint32_t limb_bits, const HostTables& h, size_t bound, size_t extra,
                 PwApcCalls& R, uint32_t* status, uint64_t* info) {
    hipStream_t st = stream();
    const size_t n_apcs = h.apcs.size();
    const size_t need = calls_need(n_states, n_states * h.max_share, h.bytes()) + extra;
    if (bound < need) {
        *status = 2;
        *info = need;
        return 0;
    }
    // small: counters of the fold (8 u64) | per-APC counters | APC table | constraints | slots — one copy per call
    std::vector<char> image;
    auto put = [&](const void* p, size_t bytes) {
        const size_t at = (image.size() + 15) & ~(size_t)15;
        image.resize(at + bytes);
        if (bytes) memcpy(image.data() + at, p, bytes);
        return at;
    };
    const std::vector<u64> zeros(8 + n_apcs * kCounters, 0);
    put(zeros.data(), zeros.size() * 8);
    const size_t at_apcs = put(h.apcs.data(), n_apcs * sizeof(ApcDev)), at_cons = put(h.cons.data(), h.cons.size() * sizeof(ConDev)),
                 at_spc = put(h.slot_pcs.data(), h.slot_pcs.size() * 4), at_sf = put(h.slot_first.data(), h.slot_first.size() * 4),
                 at_sa = put(h.slot_apcs.data(), h.slot_apcs.size() * 4);
    PW_TRY(cx.small.ensure(image.size() + 16));
    PW_HIP_TRY(hipMemcpyAsync(cx.small.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
    char* sm = cx.small.as<char>();
    u64* d_fold = (u64*)sm;
    u64* d_counters = d_fold + 8;
    uint32_t* d_n = (uint32_t*)(d_fold + 4);  // counts written by the compactions
    const Tables T{d_pcs, d_regs, n_states, limb_bits == 32u ? 0xffffffffu : (1u << limb_bits) - 1u, (const ApcDev*)(sm + at_apcs), (const ConDev*)(sm + at_cons),
                   (const uint32_t*)(sm + at_spc), (const uint32_t*)(sm + at_sf), (const uint32_t*)(sm + at_sa), (uint32_t)h.slot_pcs.size()};
    const dim3 block(kBlock);

    // ---- candidates ----
    u64 n_cand = 0;
    {
        ScopedKernelTimer timer("apc_calls_candidates");
        PW_TRY(cx.count.ensure(n_states * 4));
        PW_TRY(cx.off.ensure(n_states * 4));
        hipLaunchKernelGGL(apc_calls_match_kernel, dim3(div_up(n_states, kBlock)), block, 0, st, T, cx.count.as<uint32_t>(), d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::exclusive_scan(t, b, cx.count.as<uint32_t>(), cx.off.as<uint32_t>(), 0u, (size_t)n_states, rocprim::plus<uint32_t>(), st);
        }));
        uint32_t last[2] = {0, 0};
        PW_HIP_TRY(hipMemcpyAsync(&last[0], cx.off.as<uint32_t>() + (n_states - 1), 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(&last[1], cx.count.as<uint32_t>() + (n_states - 1), 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        n_cand = (u64)last[0] + last[1];
        cx.count.release();
        if (n_cand) {
            PW_TRY(cx.cand.ensure(n_cand * 8));
            hipLaunchKernelGGL(apc_calls_emit_kernel, dim3(div_up(n_states, kBlock)), block, 0, st, T, (const uint32_t*)cx.off.p, cx.cand.as<u64>());
            PW_HIP_TRY(hipGetLastError());
        }
    }
    cx.stat_candidates = n_cand;
    u64 n_valid = 0;
    if (n_cand) {
        // ---- validity ----
        ScopedKernelTimer timer("apc_calls_validity");
        PW_TRY(cx.item_off.ensure(n_cand * 8));
        PW_TRY(cx.fail.ensure(n_cand * 4));
        PW_TRY(cx.done.ensure(n_cand));
        PW_TRY(cx.V.ensure(n_cand * 8));
        PW_HIP_TRY(hipMemsetAsync(cx.fail.p, 0xff, n_cand * 4, st));
        const u64* d_cand = cx.cand.as<u64>();
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::exclusive_scan(t, b, rocprim::make_transform_iterator(d_cand, ChunksOf{T.apcs}), cx.item_off.as<u64>(), (u64)0, (size_t)n_cand,
                                           rocprim::plus<u64>(), st);
        }));
        u64 last_off = 0, last_cand = 0;
        PW_HIP_TRY(hipMemcpyAsync(&last_off, cx.item_off.as<u64>() + (n_cand - 1), 8, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(&last_cand, d_cand + (n_cand - 1), 8, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        const u64 n_items = last_off + h.apcs[(uint32_t)last_cand].chunks, per_launch = ((u64)1 << 30) * kBlock;
        for (u64 base = 0; base < n_items; base += per_launch)
            hipLaunchKernelGGL(apc_calls_eval_kernel, dim3(div_up(std::min(per_launch, n_items - base), kBlock)), block, 0, st, T, d_cand, (const u64*)cx.item_off.p, n_cand,
                               base, n_items, cx.fail.as<uint32_t>());
        hipLaunchKernelGGL(apc_calls_classify_kernel, dim3(div_up(n_cand, kBlock)), block, 0, st, T, d_cand, (const uint32_t*)cx.fail.p, n_cand, cx.done.as<uint8_t>(),
                           d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::select(t, b, d_cand, cx.done.as<uint8_t>(), cx.V.as<u64>(), d_n, (size_t)n_cand, st); }));
        uint32_t nv = 0;
        PW_HIP_TRY(hipMemcpyAsync(&nv, d_n, 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        n_valid = nv;
    }
    for (Scratch::Buf* b : {&cx.off, &cx.cand, &cx.item_off, &cx.fail, &cx.done}) b->release();
    cx.stat_valid = n_valid;
    std::vector<u64> calls;
    if (n_valid) {
        const u64* V = cx.V.as<u64>();
        const dim3 grid(div_up(n_valid, kBlock));
        u64 n_comp = 0;
        {
            // ---- components ----
            ScopedKernelTimer timer("apc_calls_components");
            PW_TRY(cx.end.ensure(n_valid * 4));
            PW_TRY(cx.mx.ensure(n_valid * 4));
            PW_TRY(cx.cflag.ensure(n_valid));
            PW_TRY(cx.cfirst.ensure((n_valid + 1) * 4));
            hipLaunchKernelGGL(apc_calls_ends_kernel, grid, block, 0, st, V, T.apcs, n_valid, cx.end.as<uint32_t>());
            PW_HIP_TRY(hipGetLastError());
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                return rocprim::inclusive_scan(t, b, cx.end.as<uint32_t>(), cx.mx.as<uint32_t>(), (size_t)n_valid, rocprim::maximum<uint32_t>(), st);
            }));
            hipLaunchKernelGGL(apc_calls_cut_kernel, grid, block, 0, st, V, (const uint32_t*)cx.mx.p, n_valid, cx.cflag.as<uint8_t>());
            PW_HIP_TRY(hipGetLastError());
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                return rocprim::select(t, b, rocprim::counting_iterator<uint32_t>(0), cx.cflag.as<uint8_t>(), cx.cfirst.as<uint32_t>(), d_n, (size_t)n_valid, st);
            }));
            uint32_t nc = 0;
            PW_HIP_TRY(hipMemcpyAsync(&nc, d_n, 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            n_comp = nc;
            const uint32_t total = (uint32_t)n_valid;
            PW_HIP_TRY(hipMemcpyAsync(cx.cfirst.as<uint32_t>() + n_comp, &total, 4, hipMemcpyHostToDevice, st));
            PW_HIP_TRY(hipStreamSynchronize(st));  // (total is a local)
            for (Scratch::Buf* b : {&cx.end, &cx.mx, &cx.cflag}) b->release();
        }
        cx.stat_components = n_comp;
        const u64 threshold = cx.long_threshold ? cx.long_threshold : kLongDefault, longs_cap = n_valid / (threshold + 1) + 1;
        u64 fold[2] = {0, 0};
        {
            // ---- fold ----
            ScopedKernelTimer timer("apc_calls_fold");
            PW_TRY(cx.disc.ensure(n_valid));
            PW_TRY(cx.longs.ensure(longs_cap * 4));
            PW_HIP_TRY(hipMemsetAsync(cx.disc.p, 0, n_valid, st));
            hipLaunchKernelGGL(apc_calls_fold_kernel, dim3(div_up(n_comp, kBlock)), block, 0, st, V, T.apcs, (const uint32_t*)cx.cfirst.p, n_comp, threshold,
                               cx.disc.as<uint8_t>(), cx.longs.as<uint32_t>(), longs_cap, d_fold);
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(fold, d_fold, sizeof fold, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
        }
        cx.stat_longest = std::max<u64>(fold[0], 1);
        cx.stat_long = fold[1];
        if (fold[1] > longs_cap) return (int)hipErrorInvalidValue;  // (cannot happen: more long components than candidates allow)
        if (fold[1]) {
            ScopedKernelTimer timer("apc_calls_fold_long");
            hipLaunchKernelGGL(apc_calls_fold_long_kernel, dim3((unsigned)fold[1]), dim3(64), 0, st, V, T.apcs, (const uint32_t*)cx.cfirst.p, (const uint32_t*)cx.longs.p,
                               cx.disc.as<uint8_t>());
            PW_HIP_TRY(hipGetLastError());
        }
        {
            // ---- read-out ----
            ScopedKernelTimer timer("apc_calls_readout");
            PW_TRY(cx.keep.ensure(n_valid));
            PW_TRY(cx.calls.ensure(n_valid * 8));
            hipLaunchKernelGGL(apc_calls_tally_kernel, grid, block, 0, st, V, (const uint8_t*)cx.disc.p, n_valid, cx.keep.as<uint8_t>(), d_counters);
            PW_HIP_TRY(hipGetLastError());
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::select(t, b, V, cx.keep.as<uint8_t>(), cx.calls.as<u64>(), d_n, (size_t)n_valid, st); }));
            uint32_t n_calls = 0;
            PW_HIP_TRY(hipMemcpyAsync(&n_calls, d_n, 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            calls.resize(n_calls);
            if (n_calls) PW_HIP_TRY(hipMemcpyAsync(calls.data(), cx.calls.p, (size_t)n_calls * 8, hipMemcpyDeviceToHost, st));
        }
    }
    if (n_apcs) PW_HIP_TRY(hipMemcpyAsync(R.counters.data(), d_counters, n_apcs * kCounters * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    R.ids.resize(calls.size());
    R.from.resize(calls.size());
    R.to.resize(calls.size());
    for (size_t k = 0; k < calls.size(); ++k) {
        const uint32_t a = (uint32_t)calls[k];
        R.ids[k] = a;
        R.from[k] = calls[k] >> 32;
        R.to[k] = R.from[k] + h.apcs[a].cycle;
        R.covered += h.apcs[a].cycle;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pw_apc_calls_from_states(const uint32_t* d_pcs, const uint32_t* d_regs, uint64_t n_states, uint32_t n_regs, uint32_t limb_bits, const PwApc* apcs,
                                        size_t n_apcs, const PwApcConstraint* constraints, size_t n_constraints, size_t scratch_bytes, PwApcCalls** out,
                                        uint32_t* status, uint64_t* info) {
    HostTables h;
    if (!out || !status || !info || (!d_pcs && n_states) || (!d_regs && n_regs && n_states) || n_states >= ((uint64_t)1 << 32) ||
        !check_tables(apcs, n_apcs, constraints, n_constraints, n_regs, limb_bits, h) || n_states * h.max_share >= ((uint64_t)1 << 32))
        return -1;
    AcCtx& cx = g_ac;
    const ScratchCall call(cx, out, status, info);
    auto result = empty_result(n_apcs, n_states);
    if (!n_states) {
        *out = result.release();
        return 0;
    }
    const size_t bound = call.bound(scratch_bytes);
    const int rc = select_calls(cx, d_pcs, d_regs, n_states, limb_bits, h, bound, 0, *result, status, info);
    if (!rc && !*status) *out = result.release();
    return rc;
}

extern "C" int pw_apc_calls_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, uint32_t final_pc, const PwApc* apcs,
                                        size_t n_apcs, const PwApcConstraint* constraints, size_t n_constraints, size_t scratch_bytes, PwApcCalls** out,
                                        uint32_t* status, uint64_t* info) {
    HostTables h;
    time_index::Bridge B;
    if (!out || !status || !info || bus >= bb::P || !time_index::one_segment(segment_of_air, n_airs) || !airs_well_formed(airs, n_airs) ||
        !check_tables(apcs, n_apcs, constraints, n_constraints, 0, 8, h) || !time_index::bridge_of(airs, n_airs, bus, &B) ||
        (B.M + 1) * std::max<u64>(h.max_share, 1) >= ((u64)1 << 32))
        return -1;
    const u64 M = B.M;
    AcCtx& cx = g_ac;
    const ScratchCall call(cx, out, status, info);
    hipStream_t st = stream();
    const size_t bound = call.bound(scratch_bytes);
    // the index stage holds 32 bytes per row and a sort's temporary storage; the sorted keys and the states stay through the selection
    const size_t index_need = time_index::bytes_needed(M), extra = 64 + (size_t)M * 8 + (size_t)(M + 1) * 4;
    {
        const size_t need = std::max(index_need + (size_t)(M + 1) * 4, calls_need(M + 1, (M + 1) * h.max_share, h.bytes()) + extra);
        if (bound < need) {
            *status = 2;
            *info = need;  // (what is known before a row is read: every row may be active)
            return 0;
        }
    }
    u64 N = 0;
    PW_TRY(time_index::open(airs, segment_of_air, n_airs, bus, B, cx.index, cx.temp, time_index::Names{"apc_calls_index_kernel", "apc_calls_sort_time", "apc_calls_time_kernel"},
                            &N, status, info));
    if (*status) return (int)hipGetLastError();
    // the states: the N pcs in time order and the pc after the last row
    PW_TRY(cx.states.ensure((N + 1) * 4));
    if (N) PW_HIP_TRY(hipMemcpyAsync(cx.states.p, cx.index.pc_t.p, N * 4, hipMemcpyDeviceToDevice, st));
    PW_HIP_TRY(hipMemcpyAsync(cx.states.as<uint32_t>() + N, &final_pc, 4, hipMemcpyHostToDevice, st));
    auto result = empty_result(n_apcs, N + 1);
    result->time_keys.resize(N);
    if (N) PW_HIP_TRY(hipMemcpyAsync(result->time_keys.data(), cx.index.tkey_s.p, N * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    cx.index.release();
    cx.temp.release();
    const int rc = select_calls(cx, (const uint32_t*)cx.states.p, nullptr, N + 1, 8, h, bound, 0, *result, status, info);
    if (!rc && !*status) *out = result.release();
    return rc;
}

// The trace route with registers: the states of register_states.hpp for the distinct registers the constraints name (row k of the
// table = the k-th smallest of them), the constraints' registers renamed to rows, then select_calls on the table where it lies.
extern "C" int pw_apc_calls_from_traces_registers(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, uint32_t memory_bus,
                                                  uint32_t final_pc, uint32_t reg_as, uint32_t reg_ptr_step, uint32_t n_regs, uint32_t limb_bits,
                                                  const uint32_t* initial_regs, const PwApc* apcs, size_t n_apcs, const PwApcConstraint* constraints,
                                                  size_t n_constraints, size_t scratch_bytes, PwApcCalls** out, uint32_t* status, uint64_t* info) {
    namespace rs = register_states;
    HostTables h;
    const rs::Args a{airs, segment_of_air, n_airs, bridge_bus, memory_bus, final_pc, reg_as, reg_ptr_step};
    time_index::Bridge B;
    u64 slots = 0;
    if (!out || !status || !info || !check_tables(apcs, n_apcs, constraints, n_constraints, n_regs, limb_bits, h) || !rs::args_ok(a, &B, &slots) ||
        (B.M + 1) * std::max<u64>(h.max_share, 1) >= ((u64)1 << 32))
        return -1;
    const u64 M = B.M;
    std::vector<uint32_t> regs;
    for (const ConDev& q : h.cons)
        for (const OpDev* o : {&q.l, &q.r})
            if (o->kind == 2u) regs.push_back(o->reg);
    std::sort(regs.begin(), regs.end());
    regs.erase(std::unique(regs.begin(), regs.end()), regs.end());
    if (!rs::registers_ok(regs.data(), regs.size(), reg_ptr_step)) return -1;
    std::vector<uint32_t> initial;
    for (uint32_t r : regs) {
        if (initial_regs) initial.push_back(initial_regs[r]);
    }
    for (ConDev& q : h.cons)
        for (OpDev* o : {&q.l, &q.r})
            if (o->kind == 2u) o->reg = (uint32_t)(std::lower_bound(regs.begin(), regs.end(), o->reg) - regs.begin());
    AcCtx& cx = g_ac;
    const ScratchCall call(cx, out, status, info);
    const size_t bound = call.bound(scratch_bytes);
    // the states, the table and the time keys stay through the selection
    const size_t extra = 64 + (size_t)(M + 1) * 4 * (regs.size() + 1) + (size_t)M * 8;
    {
        const size_t need = std::max(rs::bytes_needed(M, slots, regs.size()), calls_need(M + 1, (M + 1) * h.max_share, h.bytes()) + extra);
        if (bound < need) {
            *status = 2;
            *info = need;  // (what is known before a row is read: every row may be active, every interaction a send)
            return 0;
        }
    }
    u64 N = 0;
    PW_TRY(rs::states_from_traces(a, regs, initial_regs ? initial.data() : nullptr, B, slots, cx.stage, cx.states, cx.regtab, cx.tkeys, &N, status, info));
    if (*status) return (int)hipGetLastError();
    auto result = empty_result(n_apcs, N + 1);
    result->time_keys.resize(N);
    if (N) PW_HIP_TRY(hipMemcpy(result->time_keys.data(), cx.tkeys.p, N * 8, hipMemcpyDeviceToHost));
    cx.stage.release();
    const int rc = select_calls(cx, (const uint32_t*)cx.states.p, regs.empty() ? nullptr : (const uint32_t*)cx.regtab.p, N + 1, limb_bits, h, bound, 0, *result, status, info);
    if (!rc && !*status) *out = result.release();
    return rc;
}
