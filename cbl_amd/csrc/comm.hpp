// comm.hpp — the multi-GPU build behind the C ABI: a communicator (RCCL over xGMI, loaded at run time, or host callbacks
// supplied by the embedding program) and the sharded insert that runs on it. Included by cblx.cpp only (through host_input.hpp, which holds
// the PCIe ingest that feeds the one-rank routes). The first partition pass of a piece is pipeline.hpp's (first_pass_count / first_pass_scatter),
// the layout arithmetic between bin totals, headers, send ranges and piece tables is wire_layout.hpp's (host-only, unit-tested with g++).
//
// No reference counterpart (the reference is one process); the path is BASELINE.json's north_star: buckets are
// independent by prefix, so the 2^PREFIX_BITS space is cut into `world` contiguous ranges (quantiles of a sampled, all-reduced
// prefix histogram) and what the k-mers turn into crosses the links once. Three protocols, same result (byte-identical to the
// one-process build in the job's stream order, slice-major / rank-minor):
//   "bins", grouped receiver (default on an empty index; sharded_insert_grouped = the phases of GroupedInsert): the senders run KRN-1 + the FIRST partition pass on
//     bins that refine that pass's digit by the destination rank and by G groups per rank; 8-byte records + a digit byte cross the
//     links group-major, and the receiver runs the remaining passes, its window of the directory and the bucket kernels of group g
//     while groups g+1.. are still on the wire;
//   "bins", plain receiver (sharded_insert_bins = BinsInsert: non-empty index, degenerate bounds, one rank, the sliced one-GPU host input): the
//     same records slice-major, everything behind the first pass once the last record has landed;
//   "sorted" (sharded_insert_sorted): the sender partitions completely and ships prefixes, counts and packed suffixes; the receiver
//     merges the batches run by run — a third fewer bytes on the wire, one more pass over the words (2 - 4 GPUs, PREFIX_BITS <= 8).
// Transports: RCCL (grouped ncclSend / ncclRecv on a side stream), host callbacks (tests: ranks sharing one GPU), the one-rank
// local transport (a batch arriving over PCIe), and the recording / replaying pair of the one-GPU rehearsal (SimTransport).
#pragma once
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <atomic>
#include <map>
#include <functional>

#include "shard.hpp"
#include "wire_layout.hpp"

namespace {

// ---- what the sharded build needs from the wire --------------------------------------------------------------------
struct Transport {
    u32 rank = 0, world = 1;
    u64 sent_bytes = 0, recv_bytes = 0, messages = 0;
    virtual ~Transport() {}
    virtual void all_reduce_sum_u64(u64* host_vals, size_t n) = 0;                          // in place, every rank gets the sums
    virtual void all_to_all_u64(const u64* send, u64* recv, size_t per_rank) = 0;         // per_rank values to / from every rank
    // personalised exchange of byte runs in device memory: src holds the runs for rank 0..W-1 back to back (send_off[W + 1]),
    // dst receives the runs of source rank 0..W-1 back to back (recv_off[W + 1]). `after`: stream whose work produced src.
    // Returns once the exchange is ISSUED; wait() returns when everything issued so far has landed.
    virtual void exchange(const u8* d_src, const u64* send_off, u8* d_dst, const u64* recv_off, hipStream_t after) = 0;
    virtual void wait() = 0;
    // Several personalised exchanges issued as ONE (grouped receiver: a group's share of every slice and of every record array). The
    // runs of an item lie anywhere in its arrays: bytes [s_off[d], s_off[d] + s_len[d]) of src go to rank d, the bytes from rank r
    // land at [r_off[r], r_off[r] + r_len[r]) of dst; the own rank's entries are ignored (its records never leave the device).
    struct Item { const u8* src; u8* dst; std::vector<u64> s_off, s_len, r_off, r_len; };
    virtual void exchange_items(const std::vector<Item>& items, hipStream_t after) = 0;
    // `e` fires once everything issued so far has landed (`after`: the stream of a transport that completes on return)
    virtual void record(hipEvent_t e, hipStream_t after) { CBLX_HIP(hipEventRecord(e, after)); }
    virtual void begin_job() {}  // a sharded insert starts (the rehearsal transports count their calls from here)
};

// ---- RCCL, resolved at run time (librccl.so.1; a process that already loaded one — torch's — gets that one) ------------
struct Id128 { char internal[128]; };  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128 /* ncclUniqueId by value */, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
};
enum { RCCL_UINT8 = 1, RCCL_UINT64 = 5, RCCL_SUM = 0 };  // ncclUint8, ncclUint64, ncclSum (rccl.h)
RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        auto sym = [&](const char* n) { return dlsym(api.lib, n); };
        api.GetUniqueId = (int (*)(void*))sym("ncclGetUniqueId");
        api.CommInitRank = (int (*)(void**, int, Id128, int))sym("ncclCommInitRank");
        api.CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
        api.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
        api.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))sym("ncclAllReduce");
        api.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))sym("ncclSend");
        api.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))sym("ncclRecv");
        api.GroupStart = (int (*)())sym("ncclGroupStart");
        api.GroupEnd = (int (*)())sym("ncclGroupEnd");
    });
    if (!api.lib || !api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd)
        throw Error(CBLX_EDEVICE, "librccl.so.1 is not available (multi-GPU builds need RCCL)");
    return api;
}
#define CBLX_RCCL(expr)                                                                                               \
    do {                                                                                                              \
        const int _r = (expr);                                                                                        \
        if (_r != 0) throw Error(CBLX_EDEVICE, std::string("RCCL error: ") + (rccl().GetErrorString ? rccl().GetErrorString(_r) : "?") + " at " #expr); \
    } while (0)

struct RcclTransport : Transport {
    static constexpr size_t MAX_MSG = 1ull << 30;  // bytes per send / recv call
    void* comm = nullptr;
    int device = 0;
    hipStream_t cs = nullptr;      // the exchange runs on its own stream, next to the kernels of the following slice
    hipEvent_t ev = nullptr;
    u64* d_small = nullptr;        // staging for the small collectives
    size_t small_cap = 0;
    RcclTransport(const u8* id, u32 r, u32 w, int dev) {
        rank = r; world = w; device = dev;
        CBLX_HIP(hipSetDevice(dev));
        Id128 uid;
        std::memcpy(uid.internal, id, sizeof uid.internal);
        CBLX_RCCL(rccl().CommInitRank(&comm, (int)w, uid, (int)r));
        try {
            CBLX_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
            CBLX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        } catch (...) {  // a constructor that throws does not run the destructor
            if (cs) (void)hipStreamDestroy(cs);
            (void)rccl().CommDestroy(comm);
            throw;
        }
    }
    ~RcclTransport() override {
        (void)hipSetDevice(device);
        if (cs) (void)hipStreamSynchronize(cs);
        if (comm) (void)rccl().CommDestroy(comm);
        if (d_small) (void)hipFree(d_small);
        if (ev) (void)hipEventDestroy(ev);
        if (cs) (void)hipStreamDestroy(cs);
    }
    u64* small(size_t n) {
        if (small_cap < n) {
            if (d_small) { u64* old = d_small; d_small = nullptr; small_cap = 0; CBLX_HIP(hipFree(old)); }
            const size_t cap = std::max<size_t>(n, 1u << 16);
            CBLX_HIP(hipMalloc((void**)&d_small, cap * 8));
            small_cap = cap;
        }
        return d_small;
    }
    void all_reduce_sum_u64(u64* v, size_t n) override {
        u64* d = small(n);
        CBLX_HIP(hipMemcpyAsync(d, v, n * 8, hipMemcpyHostToDevice, cs));
        CBLX_RCCL(rccl().AllReduce(d, d, n, RCCL_UINT64, RCCL_SUM, comm, cs));
        CBLX_HIP(hipMemcpyAsync(v, d, n * 8, hipMemcpyDeviceToHost, cs));
        CBLX_HIP(hipStreamSynchronize(cs));
    }
    void all_to_all_u64(const u64* send, u64* recv, size_t per) override {
        u64* d = small(2 * per * world);
        u64* ds = d;
        u64* dr = d + per * world;
        CBLX_HIP(hipMemcpyAsync(ds, send, per * world * 8, hipMemcpyHostToDevice, cs));
        CBLX_RCCL(rccl().GroupStart());
        for (u32 p = 0; p < world; ++p) {
            CBLX_RCCL(rccl().Send(ds + p * per, per, RCCL_UINT64, (int)p, comm, cs));
            CBLX_RCCL(rccl().Recv(dr + p * per, per, RCCL_UINT64, (int)p, comm, cs));
        }
        CBLX_RCCL(rccl().GroupEnd());
        CBLX_HIP(hipMemcpyAsync(recv, dr, per * world * 8, hipMemcpyDeviceToHost, cs));
        CBLX_HIP(hipStreamSynchronize(cs));
    }
    void exchange(const u8* src, const u64* so, u8* dst, const u64* ro, hipStream_t after) override {
        CBLX_HIP(hipEventRecord(ev, after));
        CBLX_HIP(hipStreamWaitEvent(cs, ev, 0));
        const u32 me = rank;
        if (so[me + 1] > so[me]) CBLX_HIP(hipMemcpyAsync(dst + ro[me], src + so[me], so[me + 1] - so[me], hipMemcpyDeviceToDevice, cs));
        CBLX_RCCL(rccl().GroupStart());
        for (u32 d = 1; d < world; ++d) {  // ring order keeps the pairing of sends and receives symmetric across ranks
            const u32 to = (me + d) % world, from = (me + world - d) % world;
            for (u64 o = so[to]; o < so[to + 1]; o += MAX_MSG) { CBLX_RCCL(rccl().Send(src + o, (size_t)std::min<u64>(MAX_MSG, so[to + 1] - o), RCCL_UINT8, (int)to, comm, cs)); ++messages; }
            for (u64 o = ro[from]; o < ro[from + 1]; o += MAX_MSG) { CBLX_RCCL(rccl().Recv(dst + o, (size_t)std::min<u64>(MAX_MSG, ro[from + 1] - o), RCCL_UINT8, (int)from, comm, cs)); ++messages; }
        }
        CBLX_RCCL(rccl().GroupEnd());
        sent_bytes += so[world] - (so[me + 1] - so[me]);
        recv_bytes += ro[world] - (ro[me + 1] - ro[me]);
    }
    void wait() override { CBLX_HIP(hipStreamSynchronize(cs)); }
    void exchange_items(const std::vector<Item>& items, hipStream_t after) override {
        CBLX_HIP(hipEventRecord(ev, after));
        CBLX_HIP(hipStreamWaitEvent(cs, ev, 0));
        const u32 me = rank;
        CBLX_RCCL(rccl().GroupStart());
        for (u32 d = 1; d < world; ++d) {  // ring order, items in the same order on both ends: the k-th send to a peer meets its k-th receive
            const u32 to = (me + d) % world, from = (me + world - d) % world;
            for (const Item& it : items) {
                for (u64 o = 0; o < it.s_len[to]; o += MAX_MSG) { CBLX_RCCL(rccl().Send(it.src + it.s_off[to] + o, (size_t)std::min<u64>(MAX_MSG, it.s_len[to] - o), RCCL_UINT8, (int)to, comm, cs)); ++messages; }
                for (u64 o = 0; o < it.r_len[from]; o += MAX_MSG) { CBLX_RCCL(rccl().Recv(it.dst + it.r_off[from] + o, (size_t)std::min<u64>(MAX_MSG, it.r_len[from] - o), RCCL_UINT8, (int)from, comm, cs)); ++messages; }
            }
        }
        CBLX_RCCL(rccl().GroupEnd());
        for (const Item& it : items)
            for (u32 r = 0; r < world; ++r) if (r != me) { sent_bytes += it.s_len[r]; recv_bytes += it.r_len[r]; }
    }
    void record(hipEvent_t e, hipStream_t) override { CBLX_HIP(hipEventRecord(e, cs)); }
};

// ---- host callbacks (include/cblx.h: cblx_transport): the embedding program moves the bytes -----------------------------
struct CallbackTransport : Transport {
    cblx_transport t;
    CallbackTransport(const cblx_transport& tt, u32 r, u32 w) : t(tt) { rank = r; world = w; }
    void chk(int rc, const char* what) { if (rc != 0) throw Error(CBLX_EDEVICE, std::string("transport callback failed: ") + what); }
    void all_reduce_sum_u64(u64* v, size_t n) override { chk(t.all_reduce_sum_u64(t.user, v, n), "all_reduce_sum_u64"); }
    void all_to_all_u64(const u64* s, u64* r, size_t per) override { chk(t.all_to_all_u64(t.user, s, r, per), "all_to_all_u64"); }
    void exchange(const u8* src, const u64* so, u8* dst, const u64* ro, hipStream_t after) override {
        CBLX_HIP(hipStreamSynchronize(after));  // the callback sees finished data and is complete on return
        chk(t.exchange(t.user, src, so, dst, ro), "exchange");
        sent_bytes += so[world] - (so[rank + 1] - so[rank]);
        recv_bytes += ro[world] - (ro[rank + 1] - ro[rank]);
        messages += 2 * (world - 1);
    }
    void wait() override {}
    // the callback moves back-to-back runs: an item's runs are packed into a staging buffer, exchanged, and unpacked (tests only)
    void exchange_items(const std::vector<Item>& items, hipStream_t after) override {
        CBLX_HIP(hipStreamSynchronize(after));
        for (const Item& it : items) {
            std::vector<u64> so(world + 1, 0), ro(world + 1, 0);
            for (u32 r = 0; r < world; ++r) { so[r + 1] = so[r] + (r == rank ? 0 : it.s_len[r]); ro[r + 1] = ro[r] + (r == rank ? 0 : it.r_len[r]); }
            u8 *ts = nullptr, *tr = nullptr;
            CBLX_HIP(hipMalloc((void**)&ts, so[world] + 16));
            if (hipMalloc((void**)&tr, ro[world] + 16) != hipSuccess) { (void)hipFree(ts); throw Error(CBLX_ENOMEM, "staging buffer of the callback transport"); }
            struct Free { u8 *a, *b; ~Free() { (void)hipFree(a); (void)hipFree(b); } } fr{ts, tr};
            for (u32 r = 0; r < world; ++r) if (r != rank && it.s_len[r]) CBLX_HIP(hipMemcpy(ts + so[r], it.src + it.s_off[r], it.s_len[r], hipMemcpyDeviceToDevice));
            CBLX_HIP(hipDeviceSynchronize());
            chk(t.exchange(t.user, ts, so.data(), tr, ro.data()), "exchange");
            for (u32 r = 0; r < world; ++r) if (r != rank && it.r_len[r]) CBLX_HIP(hipMemcpy(it.dst + it.r_off[r], tr + ro[r], it.r_len[r], hipMemcpyDeviceToDevice));
            CBLX_HIP(hipDeviceSynchronize());
            sent_bytes += so[world];
            recv_bytes += ro[world];
            messages += 2 * (world - 1);
        }
    }
};

// ---- rehearsal of ONE rank of a W-GPU job on one GPU (dev / bench: tools/emulate_wire.py; cblx_comm_init_sim) ----------------------
// No multi-GPU node was available while this was built, so the schedule of the sharded insert — what the receiver's kernels hide of
// the wire — is measured on one GPU: ranks 1 .. W-1 run one after the other on a RECORDING transport that keeps what each of them
// would send to rank 0 (headers and device bytes, per call); then rank 0 runs for real on a REPLAYING transport: its collectives are
// answered from the records, and the bytes of every exchange are copied into its receive arena on a side stream that a host function
// holds back until a wire of `link_gbps` per source rank (W-1 links working in parallel, one per peer, as on an xGMI mesh) would
// have delivered them. The copies read and write what RCCL's sends and receives would read and write (HBM traffic of both
// directions); what is not emulated: the CUs RCCL's kernels occupy, and link contention. Sums over ranks are answered as W times the
// own value (the ranks of the rehearsal hold equally many reads); the group cuts travel through the store so that every rank of the
// rehearsal uses rank 1's.
struct SimStore {
    struct Buf8 { u8* p = nullptr; u64 n = 0; };
    u32 world = 0;
    u32 target = 0;  // the rank that replays (CBLX_SIM_TARGET when the store is created; 0 = the densest prefix range, W - 1 = the sparse tail)
    std::vector<std::vector<std::vector<u64>>> a2a;             // [rank][call] -> what the rank sends the target
    std::vector<std::vector<std::vector<Buf8>>> xch;            // [rank][call][item] -> bytes for rank 0
    std::vector<u32> g_bounds, g_cuts;
    bool have_cuts = false;
    ~SimStore() { for (auto& r : xch) for (auto& cl : r) for (auto& b : cl) if (b.p) (void)hipFree(b.p); }
    static std::mutex& mu() { static std::mutex m; return m; }
    // (shared ownership: a communicator keeps its store alive after cblx_sim_store_free has dropped the name)
    static std::map<u64, std::shared_ptr<SimStore>>& all() { static std::map<u64, std::shared_ptr<SimStore>> m; return m; }
    static std::shared_ptr<SimStore> get(u64 id, u32 world) {
        std::lock_guard<std::mutex> g(mu());
        auto it = all().find(id);
        if (it != all().end()) {
            if (it->second->world != world) throw Error(CBLX_EINVAL, "rehearsal store: created for another world size");
            return it->second;
        }
        if (world == 0 || world > CUT_MAX_DEST) throw Error(CBLX_EINVAL, "rehearsal store: world size out of range");
        std::shared_ptr<SimStore> p(new SimStore());
        p->world = world; p->a2a.resize(world); p->xch.resize(world);
        const char* e = std::getenv("CBLX_SIM_TARGET");
        const u32 t = e ? (u32)std::strtoul(e, nullptr, 10) : 0u;
        p->target = t < world ? t : 0u;
        all()[id] = p;
        return p;
    }
};
struct SimTransport : Transport {
    std::shared_ptr<SimStore> st;
    double link_gbps;
    size_t n_a2a = 0, n_x = 0;
    hipStream_t ps = nullptr;  // replay: the "wire"
    hipEvent_t ev = nullptr;
    struct Pace { std::chrono::steady_clock::time_point start, done; bool any = false; } pace;
    struct Gate { SimTransport* t; double seconds; bool opens; };
    std::vector<std::unique_ptr<Gate>> gates;
    SimTransport(std::shared_ptr<SimStore> s, u32 r, u32 w, double gbps) : st(std::move(s)), link_gbps(gbps) {
        rank = r; world = w;
        if (r == st->target) {
            CBLX_HIP(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
            CBLX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
    }
    ~SimTransport() override {
        if (ps) { (void)hipStreamSynchronize(ps); (void)hipStreamDestroy(ps); }
        if (ev) (void)hipEventDestroy(ev);
    }
    void begin_job() override {
        n_a2a = n_x = 0;
        if (rank != st->target) { st->a2a[rank].clear(); for (auto& cl : st->xch[rank]) for (auto& b : cl) if (b.p) (void)hipFree(b.p); st->xch[rank].clear(); }
        else { if (ps) CBLX_HIP(hipStreamSynchronize(ps)); gates.clear(); pace.any = false; }
    }
    void all_reduce_sum_u64(u64* v, size_t n) override { for (size_t i = 0; i < n; ++i) v[i] *= world; }
    void all_to_all_u64(const u64* send, u64* recv, size_t per) override {
        std::memset(recv, 0, per * world * 8);
        std::memcpy(recv + rank * per, send + rank * per, per * 8);
        const u32 tg = st->target;
        if (rank != tg) { st->a2a[rank].push_back(std::vector<u64>(send + (size_t)tg * per, send + (size_t)(tg + 1) * per)); return; }  // (what goes to the target)
        for (u32 r = 0; r < world; ++r) {
            if (r == tg) continue;
            if (st->a2a[r].size() <= n_a2a || st->a2a[r][n_a2a].size() != per) throw Error(CBLX_EINVAL, "rehearsal: rank " + std::to_string(r) + " was not recorded with this schedule");
            std::memcpy(recv + r * per, st->a2a[r][n_a2a].data(), per * 8);
        }
        ++n_a2a;
    }
    static void gate_fn(void* p) {
        Gate* g = (Gate*)p;
        Pace& pc = g->t->pace;
        const auto now = std::chrono::steady_clock::now();
        if (g->opens) { pc.start = pc.any && pc.done > now ? pc.done : now; return; }  // the wire takes the call when it is free
        pc.done = pc.start + std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(g->seconds));
        pc.any = true;
        std::this_thread::sleep_until(pc.done);
    }
    void items_common(const std::vector<Item>& items, hipStream_t after) {
        const u32 tg = st->target;
        if (rank != tg) {  // record what goes to the target
            CBLX_HIP(hipStreamSynchronize(after));
            std::vector<SimStore::Buf8> call;
            for (const Item& it : items) {
                SimStore::Buf8 b;
                b.n = it.s_len[tg];
                if (b.n) { CBLX_HIP(hipMalloc((void**)&b.p, b.n)); CBLX_HIP(hipMemcpy(b.p, it.src + it.s_off[tg], b.n, hipMemcpyDeviceToDevice)); }
                call.push_back(b);
                sent_bytes += b.n;
            }
            st->xch[rank].push_back(std::move(call));
            return;
        }
        CBLX_HIP(hipEventRecord(ev, after));
        CBLX_HIP(hipStreamWaitEvent(ps, ev, 0));
        gates.emplace_back(new Gate{this, 0.0, true});
        CBLX_HIP(hipLaunchHostFunc(ps, gate_fn, gates.back().get()));
        u64 worst = 0;
        for (u32 r = 0; r < world; ++r) {
            if (r == tg) continue;
            if (st->xch[r].size() <= n_x || st->xch[r][n_x].size() != items.size()) throw Error(CBLX_EINVAL, "rehearsal: rank " + std::to_string(r) + " was not recorded with this schedule");
            u64 from_r = 0;
            for (size_t i = 0; i < items.size(); ++i) {
                const SimStore::Buf8& b = st->xch[r][n_x][i];
                if (b.n != items[i].r_len[r]) throw Error(CBLX_EDEVICE, "rehearsal: rank " + std::to_string(r) + " recorded " + std::to_string(b.n) + " bytes, rank 0 expects " + std::to_string(items[i].r_len[r]));
                if (b.n) CBLX_HIP(hipMemcpyAsync(items[i].dst + items[i].r_off[r], b.p, b.n, hipMemcpyDeviceToDevice, ps));
                from_r += b.n;
            }
            recv_bytes += from_r;
            worst = std::max(worst, from_r);
        }
        for (const Item& it : items) for (u32 r = 0; r < world; ++r) if (r != tg) sent_bytes += it.s_len[r];
        messages += 2 * (world - 1) * items.size();
        gates.emplace_back(new Gate{this, link_gbps > 0 ? (double)worst / (link_gbps * 1e9) : 0.0, false});
        CBLX_HIP(hipLaunchHostFunc(ps, gate_fn, gates.back().get()));
        ++n_x;
    }
    void exchange_items(const std::vector<Item>& items, hipStream_t after) override { items_common(items, after); }
    void exchange(const u8* src, const u64* so, u8* dst, const u64* ro, hipStream_t after) override {
        Item it{src, dst, {}, {}, {}, {}};
        for (u32 r = 0; r < world; ++r) { it.s_off.push_back(so[r]); it.s_len.push_back(so[r + 1] - so[r]); it.r_off.push_back(ro[r]); it.r_len.push_back(ro[r + 1] - ro[r]); }
        if (so[rank + 1] > so[rank]) CBLX_HIP(hipMemcpyAsync(dst + ro[rank], src + so[rank], so[rank + 1] - so[rank], hipMemcpyDeviceToDevice, after));
        items_common(std::vector<Item>{it}, after);
    }
    void wait() override { if (ps) CBLX_HIP(hipStreamSynchronize(ps)); }
    void record(hipEvent_t e, hipStream_t after) override { CBLX_HIP(hipEventRecord(e, ps ? ps : after)); }
};
}  // namespace

struct cblx_comm {
    std::unique_ptr<Transport> t;
    int device = 0;
    u32 protocol = CBLX_PROTO_AUTO;
    u32 protocol_used = CBLX_PROTO_BINS;  // what the last sharded insert resolved AUTO to
    std::string err;
    // grouped receiver (sharded_insert_grouped): groups per rank asked for (0: CBLX_RECV_GROUPS or the default), the group cuts chosen
    // together with the bounds they refine, and how many groups the last call worked through (0: it took the ungrouped path)
    u32 recv_groups = 0, groups_used = 0;
    u32 groups_fine = 0;  // ... of which sorted 16 prefix bits behind the first pass (FINE bins, PREFIX_BITS > 24)
    std::vector<u32> g_bounds, g_cuts;
};

namespace {

// ---- splitters: quantiles of a sampled prefix histogram (necklace prefixes are heavily skewed) -----------
static const u32 SPLIT_HIST_BITS = 16, SPLIT_STRIDE = 61;
template <typename HiT>
__global__ void k_sample_hist(const u64* __restrict__ lo, const HiT* __restrict__ hi, u64 n, u32 stride, u32 shift, u32 nbits, u32* __restrict__ hist) {
    const u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * stride;
    if (i >= n) return;
    atomicAdd(&hist[get_bits(lo[i], (u64)ld_hi<HiT>(hi, i), shift, nbits)], 1u);
}
// world-1 ascending prefix values cutting the histogram mass into `world` near-equal parts (same rule as cbl_amd/sharded.py)
std::vector<u32> choose_bounds(const std::vector<u64>& hist, u32 world, u32 PB, u32 hb) {
    std::vector<u32> b;
    const size_t nh = hist.size();
    std::vector<double> cum(nh);
    double run = 0;
    for (size_t i = 0; i < nh; ++i) { run += (double)hist[i]; cum[i] = run; }
    const double total = run;
    const int shift = (int)PB - (int)hb;
    for (u32 d = 1; d < world; ++d) {
        u64 cell;
        if (total > 0) cell = (u64)(std::lower_bound(cum.begin(), cum.end(), total * d / world) - cum.begin()) + 1;
        else cell = (u64)d * nh / world;
        cell = std::min<u64>(std::max<u64>(cell, 1), nh);
        const u64 v = shift >= 0 ? std::min<u64>(cell << shift, (1ull << PB) - 1) : cell >> -shift;
        b.push_back((u32)v);
    }
    for (size_t i = 1; i < b.size(); ++i) b[i] = std::max(b[i], b[i - 1]);
    return b;
}

// the all-reduced, sampled prefix histogram (2^min(16, PB) bins) of one slice's words
template <typename C>
std::vector<u64> sampled_prefix_hist(cblx_ctx* c, Transport& T, const u8* d_bases, const u64* d_offsets, u64 nseq) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    const u32 hb = std::min(SPLIT_HIST_BITS, P.PB);
    std::vector<u64> hist((size_t)1 << hb, 0);
    if (nseq) {
        ChunkPlan pl;
        const u8* pb = d_bases;
        plan_chunks(c, pb, d_offsets, nseq, pl);
        if (pl.n_kmers) {
            Buf<u64> w_lo(c->pool, pl.n_kmers + 2);
            Buf<u8> w_hi(c->pool, (pl.n_kmers + 2) * std::max<size_t>(1, hi_elem_size(P)));
            Buf<u32> d_hist(c->pool, (size_t)1 << hb);
            CBLX_HIP(hipMemsetAsync(d_hist.get(), 0, ((size_t)1 << hb) * 4, c->stream));
            encode<C>(c, pb, pl, w_lo.get(), (HiT*)w_hi.get(), 0);
            hipLaunchKernelGGL(k_sample_hist<HiT>, grid1(ceil_div(pl.n_kmers, SPLIT_STRIDE), 256), dim3(256), 0, c->stream, w_lo.get(), (const HiT*)w_hi.get(), pl.n_kmers,
                               SPLIT_STRIDE, P.SB + P.PB - hb, hb, d_hist.get());
            CBLX_HIP(hipGetLastError());
            std::vector<u32> h32 = d2h_vec<u32>(c, d_hist.get(), (size_t)1 << hb);
            for (size_t i = 0; i < h32.size(); ++i) hist[i] = h32[i];
        }
    }
    T.all_reduce_sum_u64(hist.data(), hist.size());
    return hist;
}
// first batch only: quantile ranges from the all-reduced, sampled prefix histogram of one slice's words
template <typename C>
void choose_bounds_from_slice(cblx_ctx* c, Transport& T, const u8* d_bases, const u64* d_offsets, u64 nseq, u32* bounds, std::vector<u64>* hist_out = nullptr, u32 fine_groups = 0) {
    const Consts& P = c->P;
    const u32 hb = std::min(SPLIT_HIST_BITS, P.PB);
    std::vector<u64> hist = sampled_prefix_hist<C>(c, T, d_bases, d_offsets, nseq);
    if (fine_groups) weigh_tail_for_fine_bins(hist, P.PB, T.world, fine_groups, hb);  // (the "bins" protocol with its grouped receiver: FINE bins at PREFIX_BITS > 24)
    const std::vector<u32> bb = choose_bounds(hist, T.world, P.PB, hb);
    for (u32 d = 0; d + 1 < T.world; ++d) bounds[d] = bb[d];
    if (hist_out) *hist_out = std::move(hist);
}

// ---- what the protocols share -------------------------------------------------------------------------------------------------------
// an error between two slices must not hand the buffers of an exchange that is still running back to the pool (armed once `t` is set)
struct Drain { Transport* t; ~Drain() { if (t) try { t->wait(); } catch (...) {} } };
inline void check_slice_cuts(const u64* cuts, u32 nslices, u64 n) {
    for (u32 s = 0; s < nslices; ++s) if (cuts[s + 1] < cuts[s] || cuts[s + 1] > n) throw Error(CBLX_EINVAL, "slice cuts must be ascending and at most n");
}
static const u64 ROUND_LIMIT = 0xFFFFFFF0ull - 2 * RDX_TILE;  // one round = one batch of the pipeline (32-bit positions)

// ---- protocol "sorted": the sender partitions completely; prefixes, counts and packed suffixes on the wire; the receiver
// merges the batches run by run (fewest bytes per word: the choice when the links are the bound, world <= 4) ----------------
template <typename C>
void sharded_insert_sorted(cblx_ctx* c, Transport& T, const u8* d_bases, const u64* d_offsets, u64 n, const u64* cuts, u32 nslices, u32* bounds, int* bounds_valid) {
    const Consts& P = c->P;
    const u32 W = T.world, B = P.BYTES;
    struct Slice {
        Buf<u32> sp, sc, rp, rc;   // sent / received prefixes and counts
        Buf<u8> ss, rs;            // sent / received packed suffixes
        std::vector<u64> rb, rw;   // received buckets / words per source rank
    };
    std::vector<Slice> sl(nslices);
    Drain drain{&T};
    for (u32 s = 0; s < nslices; ++s) {
        const u64 a = cuts[s], b = cuts[s + 1];
        check_slice_cuts(cuts + s, 1, n);
        if (!*bounds_valid) {
            choose_bounds_from_slice<C>(c, T, d_bases, d_offsets + a, b - a, bounds);
            *bounds_valid = 1;
        }
        std::vector<u64> bs(W + 1), ws(W + 1);
        sorted_batch_begin<C>(c, d_bases, d_offsets + a, b - a, bounds, W, bs.data(), ws.data());
        Slice& S = sl[s];
        S.sp = Buf<u32>(c->pool, bs[W] + 1);
        S.sc = Buf<u32>(c->pool, bs[W] + 1);
        S.ss = Buf<u8>(c->pool, ws[W] * B + 16);
        sorted_batch_export<C>(c, S.sp.get(), S.sc.get(), S.ss.get());
        std::vector<u64> send(2 * W), recv(2 * W);
        for (u32 d = 0; d < W; ++d) { send[2 * d] = bs[d + 1] - bs[d]; send[2 * d + 1] = ws[d + 1] - ws[d]; }
        T.all_to_all_u64(send.data(), recv.data(), 2);
        S.rb.resize(W); S.rw.resize(W);
        std::vector<u64> so4(W + 1), ro4(W + 1), soB(W + 1), roB(W + 1);
        so4[0] = ro4[0] = soB[0] = roB[0] = 0;
        for (u32 d = 0; d < W; ++d) {
            S.rb[d] = recv[2 * d]; S.rw[d] = recv[2 * d + 1];
            so4[d + 1] = so4[d] + send[2 * d] * 4;       ro4[d + 1] = ro4[d] + S.rb[d] * 4;
            soB[d + 1] = soB[d] + send[2 * d + 1] * B;   roB[d + 1] = roB[d] + S.rw[d] * B;
        }
        S.rp = Buf<u32>(c->pool, ro4[W] / 4 + 1);
        S.rc = Buf<u32>(c->pool, ro4[W] / 4 + 1);
        S.rs = Buf<u8>(c->pool, roB[W] + 16);
        T.exchange((const u8*)S.sp.get(), so4.data(), (u8*)S.rp.get(), ro4.data(), c->stream);
        T.exchange((const u8*)S.sc.get(), so4.data(), (u8*)S.rc.get(), ro4.data(), c->stream);
        T.exchange(S.ss.get(), soB.data(), S.rs.get(), roB.data(), c->stream);
    }
    T.wait();
    std::vector<cblx_batch_view> views;  // stream order: slice-major, source-rank-minor
    for (u32 s = 0; s < nslices; ++s) {
        Slice& S = sl[s];
        u64 bo = 0, wo = 0;
        for (u32 r = 0; r < W; ++r) {
            if (S.rw[r]) views.push_back(cblx_batch_view{S.rb[r], S.rw[r], S.rp.get() + bo, S.rc.get() + bo, S.rs.get() + wo * B});
            bo += S.rb[r];
            wo += S.rw[r];
        }
        S.sp.reset(); S.sc.reset(); S.ss.reset();  // sent data is done with
    }
    if (!views.empty()) insert_sorted_batches<C>(c, views.data(), (u32)views.size());
    CBLX_HIP(hipStreamSynchronize(c->stream));
}

// ---- protocol "bins": the exchange rides between the first and the second partition pass ------------------------------------
// The sender runs KRN-1 and pass A only — on BINS (DigitBin: the pass-A segment refined by the destination rank), so its output
// is contiguous per destination and, inside a destination, per segment; the records of its own range go straight into its
// receive arena (OwnWindow), the others leave as they are: 8-byte records (the hi byte of a 65..72-bit word is implied by the
// segment, as on one GPU) plus the 1-byte digit side channel of the next pass. The receiver keeps the arena as the input of
// the remaining passes: a piece table (slice, source, segment) -> tile table of the first LSD pass (k_piece_tables), after
// which the one-GPU pipeline continues unchanged. No pass is added to the one-GPU path and no record is copied: per rank the
// job costs what the direct build costs plus the slices' fixed costs. (The bin map and the layout arithmetic: wire_layout.hpp.)
inline bool bins_protocol_fits(const Consts& P, const u32* bounds, u32 W) { return P.PB >= 9 && make_bin_map(P.PB, bounds, W).ok; }

// The receive log (arena) of the "bins" protocols: the slices land back to back — 8-byte records, the hi parts of words that keep
// one behind pass A, and the digit byte of the receiver's first LSD pass (`wire_dig`; off the wire: one block, the receiver's first
// histogram reads the records). Capacity from the job's k-mer count (an upper bound), the rank's share of it with slack for uneven
// ranges; it grows when a slice does not fit.
struct RecvLog {
    cblx_ctx* c;
    Transport& T;
    size_t ohs;            // bytes of the hi part of a record (u64 or none)
    bool wire_dig = true;  // digits on the wire
    Buf<u64> lo;
    Buf<u8> hi, dig;
    u64 cap = 0, filled = 0;
    void alloc_into(u64 ncap, Buf<u64>& l, Buf<u8>& h, Buf<u8>& dg) const {
        l = Buf<u64>(c->pool, ncap + 2);
        h = Buf<u8>(c->pool, ohs ? (ncap + 2) * ohs : 8);
        dg = Buf<u8>(c->pool, wire_dig ? ncap + 64 : 64);
    }
    void alloc() { alloc_into(cap, lo, hi, dig); }
    void grow(u64 need) {  // (grouped receiver: only own pieces and the first group's early shares are in the log)
        T.wait();
        CBLX_HIP(hipStreamSynchronize(c->stream));
        const u64 ncap = std::min<u64>(ROUND_LIMIT, need + need / 4 + 4096);
        Buf<u64> l;
        Buf<u8> h, dg;
        alloc_into(ncap, l, h, dg);
        if (filled) {
            CBLX_HIP(hipMemcpyAsync(l.get(), lo.get(), filled * 8, hipMemcpyDeviceToDevice, c->stream));
            if (ohs) CBLX_HIP(hipMemcpyAsync(h.get(), hi.get(), filled * ohs, hipMemcpyDeviceToDevice, c->stream));
            if (wire_dig) CBLX_HIP(hipMemcpyAsync(dg.get(), dig.get(), filled, hipMemcpyDeviceToDevice, c->stream));
            CBLX_HIP(hipStreamSynchronize(c->stream));
        }
        lo = std::move(l); hi = std::move(h); dig = std::move(dg);
        cap = ncap;
    }
    void room(u64 need) {  // the log holds `need` records from here on
        if (!lo.get()) alloc();
        if (need > cap) grow(need);
    }
    void reset() { lo.reset(); hi.reset(); dig.reset(); }
    // where the first pass writes the sender's own records: the end of the log
    OwnWindow own_window(const OwnShare& own) const {
        return OwnWindow{own.a, own.a + own.n, lo.get() + filled, ohs ? (void*)(hi.get() + filled * ohs) : nullptr, wire_dig ? dig.get() + filled : (u8*)nullptr};
    }
};

// One rank: the bin totals of a first pass that stay on the device until the passes of the round are queued (no host round trip between
// KRN-1 and the pass), then become the piece's row of the piece table. `what`: "slice" or "piece" (the text of the count check).
struct DeferredTotals { size_t piece; u64 n; Buf<u32> coltot; };
template <typename Map> void fold_deferred(cblx_ctx* c, const Map& M, std::vector<DeferredTotals>& v, const char* what, std::vector<u32>& pcnt) {
    for (DeferredTotals& d : v) {
        const std::vector<u32> t = d2h_vec<u32>(c, d.coltot.get(), 256);
        std::vector<u64> row(WIRE_HDR, 0);
        wire_header(M, t.data(), 1, 0, d.n, what, row.data());
        for (u32 cl = 0; cl < 256; ++cl) pcnt[d.piece * 256 + cl] += (u32)row[1 + cl];
    }
    v.clear();
}

// One call of sharded_insert_bins (below): the slices one by one, the round's end.
template <typename C>
struct BinsInsert {
    typedef typename C::HiT HiT;
    static constexpr bool DROP_HI = std::is_same<HiT, u8>::value;
    typedef typename std::conditional<DROP_HI, NoHi, HiT>::type OutH;  // record layout behind pass A
    static constexpr size_t OHS = HiTraits<OutH>::has ? sizeof(u64) : 0;  // bytes of the hi part on the wire (u64 or none)
    cblx_ctx* c;
    Transport& T;
    const u32 W, me;
    const BinMap M;
    DigitBin fn;
    EncHist eh0{};
    DigitBits nextd;
    const bool trace = std::getenv("CBLX_TRACE_SHARDED") != nullptr;
    u64 mine, job;
    RecvLog log;
    // send buffers of the exchanges in flight. A slice's buffers go back to the pool as soon as its exchange has completed (an event
    // behind it on the transport's stream, polled at the start of every later slice): what stays allocated is bounded by the slices the
    // wire is behind, not by the job (a whole call's send buffers — (W-1)/W of the rank's words, 9 bytes each — next to the receive
    // arena and the pipeline's twin could run one rank out of memory while the others wait in a collective)
    struct Sent { Buf<u64> lo; Buf<u8> hi, dig; hipEvent_t done = nullptr; };
    std::vector<Sent> sent;
    struct SentEvents { std::vector<Sent>& v; ~SentEvents() { for (Sent& x : v) if (x.done) (void)hipEventDestroy(x.done); } } sent_events{sent};
    std::vector<u32> pcnt, pbase;      // piece table of the round: [piece][256] counts, arena position of every piece
    FirstPass prev_work;  // workspace of the previous slice
    // one rank (a batch arriving over PCIe, insert_device_sliced): everything is the rank's own, nothing has to be agreed per slice —
    // the bin counts of a slice stay on the device until the round ends, and the slices run without a host round trip between
    // KRN-1 and pass A
    std::vector<DeferredTotals> deferred;
    Drain drain{nullptr};

    // `mine_`: an upper bound of this rank's k-mers — the job's count (all-reduced) gives the capacity of the log
    BinsInsert(cblx_ctx* ctx, Transport& t, const u32* bounds, u64 mine_) : c(ctx), T(t), W(t.world), me(t.rank), M(make_bin_map(ctx->P.PB, bounds, t.world)), mine(mine_), job(mine_), log{ctx, t, OHS} {
        const Consts& P = c->P;
        const LsdPlan LP = lsd_plan(P, false);  // (the receiver runs LSD passes only: pipeline.hpp)
        nextd = DigitBits{P.SB + LP.sh[0], LP.wid[0]};
        fn.SB = P.SB; fn.PB = P.PB; fn.RB = P.PB - 8; fn.nd = W;
        eh0.nd = W; eh0.SB = P.SB; eh0.PB = P.PB; eh0.binRB = P.PB - 8;
        for (u32 i = 0; i < MAX_DEST - 1; ++i) { fn.bounds[i] = i + 1 < W ? bounds[i] : 0xFFFFFFFFu; eh0.bounds[i] = fn.bounds[i]; }
        T.all_reduce_sum_u64(&job, 1);
        const u64 cap = W == 1 ? mine : std::min<u64>(job, job / W + job / (4 * W) + (1u << 20));
        log.cap = std::min<u64>(std::max<u64>(cap, 1024), ROUND_LIMIT);
        drain.t = &T;
    }
    void reap_sent() {
        for (size_t i = 0; i < sent.size();) {
            if (sent[i].done && hipEventQuery(sent[i].done) == hipSuccess) {
                (void)hipEventDestroy(sent[i].done);
                sent[i] = std::move(sent.back());
                sent.pop_back();
            } else { (void)hipGetLastError(); ++i; }
        }
    }
    // what has been received so far goes through the rest of the pipeline (end of the call, or the arena would pass 2^32 records)
    void finish_round() {
        T.wait();
        CBLX_HIP(hipStreamSynchronize(c->stream));
        for (Sent& x : sent) if (x.done) { (void)hipEventDestroy(x.done); x.done = nullptr; }
        sent.clear();
        if (trace) fprintf(stderr, "[cblx bins] rank %u round ends: filled=%llu pieces=%zu\n", me, (unsigned long long)log.filled, pbase.size());
        fold_deferred(c, M, deferred, "slice", pcnt);
        if (log.filled) {
            Records rec;
            rec.lo = std::move(log.lo); rec.hi = std::move(log.hi);
            rec.lo2 = Buf<u64>(c->pool, log.filled + 2); rec.hi2 = Buf<u8>(c->pool, OHS ? (log.filled + 2) * OHS : 8);
            PieceInput pin;
            pin.np = (u32)pbase.size(); pin.cnt = pcnt.data(); pin.pbase = pbase.data(); pin.dig = &log.dig;
            pipeline<C>(c, rec, log.filled, Buf<u32>(), &pin);
            c->kmers_inserted += log.filled;
        }
        log.reset();
        pcnt.clear(); pbase.clear();
        log.filled = 0;
    }
    // slice s = `nseq` sequences from d_off: KRN-1 + pass A on bins, the count exchange, the own piece into the log, the rest onto the wire
    void slice(u32 s, const BaseView& d_bases, const u64* d_off, u64 nseq) {
        reap_sent();
        // -- KRN-1 with the bin histogram fused in, column prefixes of pass A
        ChunkPlan pl;
        BaseView pb = d_bases;
        u64 N = 0;
        if (nseq) { plan_chunks(c, pb, d_off, nseq, pl); N = pl.n_kmers; }  // (ends with a stream synchronisation)
        else CBLX_HIP(hipStreamSynchronize(c->stream));
        prev_work = FirstPass();  // the previous slice's kernels are done: its workspace goes back to the pool
        if (N >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "one slice takes fewer than 2^32-16 words (use more slices)");
        FirstPass wk;
        wk.pl = std::move(pl);
        std::vector<u32> tot(256, 0u);
        if (N) {
            first_pass_count<C>(c, wk, pb, wk.pl, N, eh0);
            if (W > 1) tot = d2h_vec<u32>(c, wk.coltot.get(), 256);
        }
        // -- what goes where: per destination the word count and the count of every segment (header of the exchange)
        const size_t HDR = WIRE_HDR;
        std::vector<u64> send((size_t)W * HDR, 0), recv((size_t)W * HDR, 0);
        OwnShare own;
        if (W == 1) { send[0] = N; recv[0] = N; own.n = N; }  // (the segment counts follow at the end of the round: `deferred`)
        else own = wire_header(M, tot.data(), W, me, N, "slice", send.data());
        if (W > 1) T.all_to_all_u64(send.data(), recv.data(), HDR);
        u64 incoming = 0;
        if (recv[(size_t)me * HDR] != own.n) throw Error(CBLX_EDEVICE, "sharded build: the count exchange returned another own count (transport error)");
        for (u32 r = 0; r < W; ++r) incoming += recv[(size_t)r * HDR];
        if (incoming >= ROUND_LIMIT) throw Error(CBLX_ERANGE, "one slice of the job sends this rank 2^32 words or more (use more slices)");
        if (trace) fprintf(stderr, "[cblx bins] rank %u slice %u: N=%llu own=%llu incoming=%llu filled=%llu cap=%llu mine=%llu job=%llu\n", me, s, (unsigned long long)N, (unsigned long long)own.n,
                           (unsigned long long)incoming, (unsigned long long)log.filled, (unsigned long long)log.cap, (unsigned long long)mine, (unsigned long long)job);
        if (log.filled + incoming > ROUND_LIMIT) finish_round();
        log.room(log.filled + incoming);
        const u64 filled = log.filled;
        // -- arena layout of the slice: the own piece first (pass A writes it there), then the other sources in rank order
        std::vector<u64> so(W + 1, 0), ro(W + 1, 0);  // record positions in the send buffer / behind the own piece
        for (u32 d = 0; d < W; ++d) {
            so[d + 1] = so[d] + (d == me ? 0 : send[(size_t)d * HDR]);
            ro[d + 1] = ro[d] + (d == me ? 0 : recv[(size_t)d * HDR]);
        }
        push_pieces(recv.data(), W, me, filled, own.n, pbase, pcnt);
        if (W == 1 && N) deferred.push_back(DeferredTotals{pbase.size() - 1, N, std::move(wk.coltot)});
        Sent S;
        log.alloc_into(N - own.n, S.lo, S.hi, S.dig);  // (a send buffer is laid out as the log is)
        if (N) first_pass_scatter<HiT, OutH, DigitBin, true>(c, wk, wk.t_lo.get(), (const HiT*)wk.t_hi.get(), fn, S.lo.get(), (OutH*)S.hi.get(), true, nextd, S.dig.get(), log.own_window(own));
        // -- the exchange (on the transport's stream, behind pass A): records, hi parts, digits
        std::vector<u64> sob(W + 1), rob(W + 1);
        auto xchg = [&](const u8* src, u8* dst, size_t es) {
            for (u32 d = 0; d <= W; ++d) { sob[d] = so[d] * es; rob[d] = ro[d] * es; }
            T.exchange(src, sob.data(), dst, rob.data(), c->stream);
        };
        if (W > 1) {
            xchg((const u8*)S.lo.get(), (u8*)(log.lo.get() + filled + own.n), 8);
            if (OHS) xchg(S.hi.get(), log.hi.get() + (filled + own.n) * OHS, OHS);
            xchg(S.dig.get(), log.dig.get() + filled + own.n, 1);
        }
        log.filled += incoming;
        if (W > 1) {
            CBLX_HIP(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
            T.record(S.done, c->stream);
        }
        sent.push_back(std::move(S));
        // the slice's workspace (chunk plan, words, count matrix) stays until the next slice's chunk plan has synchronised the
        // stream: the host queues the next slice's first kernels while this slice's pass A is still running
        prev_work = std::move(wk);
    }
};
// `before_slice` (optional): called before slice s is touched — where a caller whose slices are still arriving (a batch on its way
// over PCIe, flush()) makes the ctx's stream wait for slice s; before_slice(~0u) precedes the first read of the offsets.
template <typename C, typename Hook>
void sharded_insert_bins(cblx_ctx* c, Transport& T, const BaseView& d_bases, const u64* d_offsets, u64 n, const u64* cuts, u32 nslices, const u32* bounds, Hook&& before_slice) {
    check_slice_cuts(cuts, nslices, n);
    before_slice(~0u);
    BinsInsert<C> J(c, T, bounds, kmers_upper_bound(c, d_offsets, cuts[0], cuts[nslices]));
    for (u32 s = 0; s < nslices; ++s) {
        before_slice(s);
        J.slice(s, d_bases, d_offsets + cuts[s], cuts[s + 1] - cuts[s]);
    }
    J.finish_round();
    CBLX_HIP(hipStreamSynchronize(c->stream));
}

// ---- protocol "bins" with a GROUPED receiver: the wire hidden behind the receiver's own kernels ---------------------------------
// In sharded_insert_bins the remaining passes and the bucket kernels start when the LAST record has landed: at 8 GPUs the wire
// (25 - 30 ms) lies bare in front of 27 - 36 ms of receiver kernels. Here every rank's prefix range is cut into G groups of about
// equal sampled mass (choose_group_cuts) and the senders' first pass runs on bins that refine the pass-A segment by ALL cuts
// (DigitCut) — so a sender's output is contiguous per (destination, group), and inside that per segment, as before. The senders
// finish KRN-1 + pass A of all their slices first (10 - 12 ms during which the wire idles, but the GPU does not); then the data
// crosses GROUP-MAJOR: one grouped send / receive per group, carrying that group's share of every slice. The receive log is laid
// out exactly as before (slice-major, source-minor pieces, each sorted by bin), only the order of arrival changes: when group g
// has landed (an event on the transport's stream) its records — pieces of the log — go through the LSD passes, their window of the
// directory and the bucket kernels into the group's slot of the final arena (pipeline_group) while groups g + 1 .. are still on the
// wire. Per group the receiver's kernels take about as long as the group's bytes need on 7 links, so from the first group on the
// GPU is the bound. Inside a group a segment value occurs in one bin only (every cut is a group or rank boundary), so the group's
// piece table is the old one with other counts. Declines (returns false, identically on every rank: the decision rests on
// replicated values only) when the index is not empty anywhere, the cuts do not fit the table, or a rank's share needs two rounds.
__global__ void k_add_u64(u64* __restrict__ v, u64 n, u64 add) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] += add;
}
// batches from this many k-mers (an upper bound of them) on take the FINE-bins build on one GPU; CBLX_FINE_MIN overrides (tests: 0)
u64 fine_min_words() {  // read per call: tests switch it
    const char* e = std::getenv("CBLX_FINE_MIN");
    return e ? std::strtoull(e, nullptr, 10) : (u64)(4u << 20);
}
// What CBLX_PROTO_AUTO resolves to on `world` ranks (cblx.h): between 2 and 4 GPUs every pair shares ONE link and the words of "bins" / "sorted" are
// bound by it — on 2 and 3 ranks the reads themselves cross ("replicate": 49.8 / 61.9 ms per step at cfg 3 and 55 GB/s per link against 101.3 / 76.7
// "sorted" and 127 / 89.8 "bins", profiles/r06_wire_emulated.md); on 4 the W encodes of "replicate" cost more than the packed suffixes of "sorted"
// (74.7 against 69.1); from 5 ranks on the receiver's kernels are the bound and "bins" adds no pass.
inline u32 auto_protocol(u32 world) { return world >= 2 && world <= 3 ? CBLX_PROTO_REPLICATE : (world == 4 ? CBLX_PROTO_SORTED : CBLX_PROTO_BINS); }
inline u32 recv_groups_wanted(const cblx_comm* cm) {
    if (cm->recv_groups) return cm->recv_groups;
    const char* e = std::getenv("CBLX_RECV_GROUPS");
    const u32 v = e ? (u32)std::strtoul(e, nullptr, 10) : 0;
    if (v) return std::min(v, 14u);
    // "replicate" has no wire for its groups to hide: two of them (the FINE bins still want the dense part of the range apart from the tail) — 48.2
    // against 49.0 ms with four at cfg 3 on two ranks
    const u32 proto = cm->protocol == CBLX_PROTO_AUTO && cm->t ? auto_protocol(cm->t->world) : cm->protocol;
    if (proto == CBLX_PROTO_REPLICATE) return 2u;
    return 4u;  // measured against a paced wire (profiles/r04_wire_emulated.md): 4 groups are best at 55 GB/s per link for every configuration; more pay on slower links
}
// The "replicate" protocol (sharded_insert_replicate below): the READS of every rank as this rank holds them after the all-gather — the own ones
// as the caller's ASCII bytes, the peers' as bit planes indexed by the sender's base positions — with every rank's slice cuts.
struct ReplicaSource {
    BaseView view{nullptr, nullptr, nullptr};
    const u64* d_off = nullptr;  // nseq + 1 offsets (the sender's own positions)
    u64 nseq = 0;
    std::vector<u64> cuts;       // nslices + 1 sequence indices relative to d_off
};
struct Replica {
    std::vector<ReplicaSource> src;
    // every slice in `parts` parts (the cuts of a source then hold nslices * parts + 1 entries): the peers' planes cross the links part by part and
    // a peer's part is transformed as soon as part_ready[t] has fired (null / empty: nothing to wait for). Stream order stays slice-major, rank-minor,
    // part-minor: parts only cut the pieces, they do not reorder them.
    u32 parts = 1;
    std::vector<hipEvent_t> part_ready;
    // a batch that is still ARRIVING (one rank, insert_device_sliced: slices land over PCIe): every slice is planned on its own once `ready(s)` has
    // made the stream wait for it (s = ~0u: the offsets' first and last entry)
    bool per_slice = false;
    std::function<void(u32)> ready;
};
// One call of the grouped insert, phase by phase (sharded_insert_grouped below runs them in order).
// `single`: ONE rank whose "groups" are the part of the prefix space the FINE bins cover in blocks of 2^16 prefixes and the rest (insert_device_fine):
// no wire, the same sender and receiver steps
// `rep`: no records cross the wire — piece (slice, source) is what THIS rank's first pass keeps of the source's reads (its own prefix range), the
// receiver steps are the same
template <typename C>
struct GroupedInsert {
    typedef typename C::HiT HiT;
    static constexpr bool WS = C::WS;
    static constexpr bool DROP_HI = std::is_same<HiT, u8>::value;
    typedef typename std::conditional<DROP_HI, NoHi, HiT>::type OutH;
    static constexpr size_t OHS = HiTraits<OutH>::has ? sizeof(u64) : 0;
    static constexpr size_t HDR = WIRE_HDR;
    // -- the call (the job is an aggregate: these ten are given, the rest follows from them)
    cblx_ctx* c; cblx_comm* cm; const u8* d_bases; const u64* d_offsets; u64 n; const u64* cuts; u32 nslices; const u32* bounds; bool single; const Replica* rep;
    Transport& T = *cm->t;
    const Consts& P = c->P;
    const u32 W = T.world, me = T.rank, RB = P.PB - 8, G = recv_groups_wanted(cm);
    // -- what resolve() settles
    FinePlan FM;
    CutPlan LM;
    bool fine = false, wire_dig = false;
    const bool trace = std::getenv("CBLX_TRACE_SHARDED") != nullptr;
    u64 mine = 0, job = 0;
    DigitBits nextd{0, 0};
    Buf<u32> d_tab;  // CutCell[CUT_KEYS], or u32[FINE_CELLS]: staged in LDS by the kernels that look bins up
    DigitCut fn{};
    EncHist eh0{};
    u32 my_lo = 0, my_cells = 0, NG = 0, Gmax = 0;
    std::vector<u32> gc0;  // cells (= my bins) of every one of my groups
    // -- the senders' side
    RecvLog log{c, T, OHS};
    struct Sent { Buf<u64> lo; Buf<u8> hi, dig; std::vector<u32> tot; OwnShare own; };
    std::vector<Sent> sent;
    std::vector<u32> pcnt, pbase;  // [piece][256] records per CELL of mine, log position of every piece; piece = slice * W + source
    std::vector<std::vector<u64>> recvh;  // headers: what every source sends me, per slice
    Drain drain{nullptr};
    EventOwner gev;  // gev.e[k] fires when group k of every rank has landed
    FirstPass prev_work;
    // ONE chunk plan for the call, the slices are ranges of it (a plan per slice cost the send phase 0.4 ms of host round trips each)
    ChunkPlan PL;
    BaseView pb = ascii_view(d_bases);
    std::vector<PlanSlice> psl;
    // -- the receiver's side
    Resident fin;
    Buf<u64> fin_hi_keep;  // 16-byte records through the passes: a target for the hi parts even when the arena keeps none
    u64* fin_hi = nullptr;
    std::vector<u64> gN, gbase;  // words of every group of mine, their slots in the final arena
    std::vector<Resident> parts;

    const CutPlan& plan() const { return fine ? static_cast<const CutPlan&>(FM) : LM; }

    // FINE plan or cut plan, the job's size and the switches agreed between the ranks; false: the call is not for this route
    bool resolve() {
        cm->groups_used = cm->groups_fine = 0;
        if ((W < 2 && !single) || W > MAX_DEST || G < 2 || P.PB < 9 || nslices == 0) return false;
        check_slice_cuts(cuts, nslices, n);
        // -- the group cuts that go with these bounds (chosen once per set of bounds: a sampled histogram of the first slice, all-reduced)
        const std::vector<u32> bvec(bounds, bounds + (W - 1));
        if (!single && cm->g_bounds != bvec) {
            std::vector<u64> hist = sampled_prefix_hist<C>(c, T, d_bases, d_offsets + cuts[0], cuts[1] - cuts[0]);
            weigh_tail_for_fine_bins(hist, P.PB, W, G, std::min(SPLIT_HIST_BITS, P.PB));
            cm->g_cuts = choose_group_cuts(hist, bounds, W, G, P.PB);
            cm->g_bounds = bvec;
        }
        // PREFIX_BITS > 24: FINE bins (cuts.hpp) — the first pass also cuts the narrow groups into aligned blocks of 2^16 prefixes, so their
        // receiver sorts 16 bits in two LSD passes instead of 20 in three (CBLX_FINE_BINS=0: the bins of the top 8 prefix bits, as below 25)
        // every bin must imply the prefix bits a record does not carry behind the first pass: 65..72-bit words travel as their low 64 bits
        const u32 lmax = DROP_HI ? std::min(24u, 64u - P.SB) : 24u;
        if (P.PB > 24 && fine_bins_enabled()) FM = make_fine_plan(P.PB, lmax, bounds, W, cm->g_cuts, single);
        fine = FM.ok;
        if (single && !fine) return false;
        if (!fine) LM = make_cut_plan(P.PB, bounds, W, cm->g_cuts);
        const CutPlan& M = plan();
        // -- the job: k-mers per rank (upper bound), whether any rank holds an index already
        if (rep && rep->ready) rep->ready(~0u);
        mine = kmers_upper_bound(c, d_offsets, cuts[0], cuts[nslices]);
        // (every term of the decision below is replicated: a rank that alone holds 2^32 k-mers says so through the sum)
        // The digit side channel of the receiver's first LSD pass (1 byte per word) stays OFF the wire by default (round 5): at 8 GPUs and 55 GB/s per
        // link the step is bound by the wire from the first group on (DESIGN_HISTORY.md §5.8), the byte is a ninth of it, and the receiver's first histogram
        // reads the records instead (8 bytes per word where it read 1: about the millisecond the senders' byte stores cost). CBLX_WIRE_DIGITS=1 sends
        // it as rounds 3 - 4 did; one rank (no wire) always keeps it.
        const char* wd_env = std::getenv("CBLX_WIRE_DIGITS");
        wire_dig = single || rep != nullptr || (wd_env && wd_env[0] == '1');
        // What crosses the wire follows from switches every rank reads in its OWN environment (CBLX_FINE_BINS, CBLX_WIRE_DIGITS, CBLX_FINE_TAIL_WEIGHT,
        // CBLX_RECV_GROUPS): they are job-wide. A rank started with other values would wait for items its peers never send, or bin records by another
        // table — so the resolved choices ride in the all-reduce below (sum and sum of squares: equal on every rank iff W x sum(v^2) = sum(v)^2).
        const u64 choice = (fine ? 1ull : 0ull) | (wire_dig ? 2ull : 0ull) | ((u64)G << 2) | (std::min<u64>(fine_tail_weight_pct(), 0xFFFFull) << 8);
        u64 agree[5] = {mine, c->res.count != 0 ? 1ull : 0ull, mine >= ROUND_LIMIT ? 1ull : 0ull, choice, choice * choice};
        T.all_reduce_sum_u64(agree, 5);
        if (agree[4] * W != agree[3] * agree[3])
            throw Error(CBLX_EINVAL, "sharded build: the ranks resolved CBLX_FINE_BINS / CBLX_WIRE_DIGITS / CBLX_FINE_TAIL_WEIGHT / CBLX_RECV_GROUPS differently (they are job-wide: set them in every rank's environment)");
        job = agree[0];
        if (!M.ok || agree[1] != 0 || agree[2] != 0 || job / W + job / (2 * W) + (1u << 20) >= ROUND_LIMIT) return false;
        if (single && mine < fine_min_words()) return false;  // (a small batch: the groups' fixed costs outweigh the pass saved)
        const LsdPlan LP = fine ? lsd_plan_bits(FINE_LEVEL) : lsd_plan(P, false);  // (the receiver runs LSD passes only: pipeline.hpp; FINE bins: the first digit is the same for 16 and 24 sorted bits)
        nextd = wire_dig ? DigitBits{P.SB + LP.sh[0], LP.wid[0]} : DigitBits{0, 0};
        d_tab = Buf<u32>(c->pool, DigitCut::LDS_WORDS);
        if (fine) h2d(c, d_tab.get(), FM.tab32.data(), FM.tab32.size());
        else h2d(c, d_tab.get(), reinterpret_cast<const u32*>(M.tab.data()), M.tab.size() * 2);
        fn = DigitCut{P.SB, P.PB, RB, d_tab.get(), fine ? FM.ksh : 0xFFFFFFFFu};
        eh0.nd = W; eh0.SB = P.SB; eh0.PB = P.PB; eh0.binRB = RB; eh0.cut_tab = d_tab.get(); eh0.cut_ksh = fn.ksh;
        if (single && fine) {
            // one rank: the plan is regular — multiples of 2^16 up to the one group cut, multiples of 2^lmax above — and the bin is arithmetic
            // (checked against the plan's table, cell by cell; the table route stays for anything else)
            const u32 x = cm->g_cuts[0];
            bool regular = (x & 0xFFFFu) == 0;
            for (u32 k = 0; regular && k < FINE_CELLS; ++k) {
                const u32 p = k << FM.ksh, b = ((p < x ? p : x) >> 16) + (p >= x ? (p >> lmax) - (x >> lmax) : 0u);
                regular = (FM.tab32[k] >> 8) == FINE_NO_CUT && (FM.tab32[k] & 255u) == b;
            }
            if (regular) { fn.reg_x = x; fn.reg_lmax = lmax; fn.tab = nullptr; eh0.reg_x = x; eh0.reg_lmax = lmax; eh0.cut_tab = nullptr; }
        }
        my_lo = M.bin_lo[me]; my_cells = M.bin_lo[me + 1] - M.bin_lo[me]; NG = M.ngroups[me];
        gc0 = group_cells(M, me);
        for (u32 d = 0; d < W; ++d) Gmax = std::max(Gmax, M.ngroups[d]);
        log.wire_dig = wire_dig;
        log.cap = std::min<u64>(std::max<u64>(std::min<u64>(job, job / W + job / (4 * W) + (1u << 20)), 1024), ROUND_LIMIT);
        sent.resize(nslices); recvh.resize(nslices); psl.resize(nslices);
        gev.e.assign(Gmax, nullptr);
        drain.t = &T;
        return true;
    }

    // the items of (group k, slice s): this rank's records for every other rank's group k, and where the other ranks' records for
    // this rank's group k land in the log (every rank issues the same items in the same order, empty ones included: a callback
    // transport's exchange is a collective)
    void add_items(u32 k, u32 s, std::vector<Transport::Item>& items) {
        const CutPlan& M = plan();
        Sent& S = sent[s];
        std::vector<u64> so(W, 0), sl(W, 0), rof(W, 0), rl(W, 0);
        for (u32 d = 0; d < W; ++d) {
            if (d == me || k >= M.ngroups[d]) continue;
            u32 b0, b1;  // bins of (rank d, group k)
            group_bins(M, d, k, b0, b1);
            if (b0 >= b1) continue;
            send_range(S.tot.data(), S.own, b0, b1, so[d], sl[d]);
        }
        if (k < NG)
            for (u32 r = 0; r < W; ++r) {
                if (r == me) continue;
                u64 before;
                count_range(pcnt.data() + ((size_t)s * W + r) * 256, gc0[k], gc0[k + 1], before, rl[r]);
                rof[r] = (u64)pbase[(size_t)s * W + r] + before;
            }
        auto item = [&](const u8* src, u8* dst, size_t es) {
            Transport::Item it{src, dst, so, sl, rof, rl};
            for (u32 r = 0; r < W; ++r) { it.s_off[r] *= es; it.s_len[r] *= es; it.r_off[r] *= es; it.r_len[r] *= es; }
            items.push_back(std::move(it));
        };
        item((const u8*)S.lo.get(), (u8*)log.lo.get(), 8);
        if (OHS) item(S.hi.get(), log.hi.get(), OHS);
        if (wire_dig) item(S.dig.get(), log.dig.get(), 1);
    }

    // -- senders, records on the wire: KRN-1 + pass A of every slice; the own records go straight into the log, the rest waits in the
    //    slice's send buffer. Group 0 of every slice but the last leaves under the next slice's kernels; then the wire, group-major.
    void send_wire() {
        const u64 n0 = cuts[0], n1 = cuts[nslices];
        if (n1 > n0) {
            std::vector<u64> marks(nslices + 1);
            for (u32 s = 0; s <= nslices; ++s) marks[s] = cuts[s] - n0;
            plan_chunks(c, pb, d_offsets + n0, n1 - n0, PL, nullptr, &marks, &psl);
        }
        for (u32 s = 0; s < nslices; ++s) {
            wire_slice(s);
            if (s + 1 < nslices) {  // the first group's share of this slice crosses the links under the next slice's kernels
                std::vector<Transport::Item> items;
                add_items(0, s, items);
                T.exchange_items(items, c->stream);
            }
        }
        // -- the wire, group-major: exchange k carries group k of EVERY rank (ranks with fewer groups send nothing in the later ones)
        for (u32 k = 0; k < Gmax; ++k) {
            std::vector<Transport::Item> items;
            // (group 0 of every slice but the last left right behind that slice's pass A, under the next slice's kernels)
            for (u32 s = (k == 0 ? nslices - 1 : 0u); s < nslices; ++s) add_items(k, s, items);
            T.exchange_items(items, c->stream);
            CBLX_HIP(hipEventCreateWithFlags(&gev.e[k], hipEventDisableTiming));
            T.record(gev.e[k], c->stream);
        }
    }
    void wire_slice(u32 s) {
        const CutPlan& M = plan();
        const u64 N = psl[s].k_hi - psl[s].k_lo;
        prev_work = FirstPass();  // (its kernels are queued on this stream in front of whatever takes the blocks next)
        if (N >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "one slice takes fewer than 2^32-16 words (use more slices)");
        FirstPass wk;
        Sent& S = sent[s];
        S.tot.assign(256, 0u);
        if (N) {
            first_pass_count<C>(c, wk, pb, PL, N, eh0, &psl[s]);
            S.tot = d2h_vec<u32>(c, wk.coltot.get(), 256);
        }
        // header per destination: words, then words per cell of the destination's range
        std::vector<u64> send((size_t)W * HDR, 0);
        recvh[s].assign((size_t)W * HDR, 0);
        S.own = wire_header(M, S.tot.data(), W, me, N, "slice", send.data());
        T.all_to_all_u64(send.data(), recvh[s].data(), HDR);
        const std::vector<u64>& recv = recvh[s];
        u64 incoming = 0;
        if (recv[(size_t)me * HDR] != S.own.n) throw Error(CBLX_EDEVICE, "sharded build: the count exchange returned another own count (transport error)");
        for (u32 r = 0; r < W; ++r) incoming += recv[(size_t)r * HDR];
        {   // a share that needs two rounds is an error of the JOB: every rank learns of it here and leaves together (a rank that threw on
            // its own left its peers waiting in the next collective until the launcher's deadline)
            u64 over = log.filled + incoming >= ROUND_LIMIT ? 1ull : 0ull;
            T.all_reduce_sum_u64(&over, 1);
            if (over) throw Error(CBLX_ERANGE, "a rank's share of the job takes more than one round: set CBLX_RECV_GROUPS=1 (ungrouped receiver) or use more ranks");
        }
        log.room(log.filled + incoming);
        const u64 filled = log.filled;
        push_pieces(recv.data(), W, me, filled, S.own.n, pbase, pcnt);  // (log layout of the slice as in sharded_insert_bins)
        log.alloc_into(N - S.own.n, S.lo, S.hi, S.dig);  // (a send buffer is laid out as the log is)
        if (N) {
            if (single)  // one rank: every record is its own, the pass writes the log directly (measured: the redirecting instantiation costs the same)
                first_pass_scatter<HiT, OutH, DigitCut, false>(c, wk, wk.t_lo.get(), (const HiT*)wk.t_hi.get(), fn, log.lo.get() + filled, OHS ? (OutH*)(log.hi.get() + filled * OHS) : (OutH*)nullptr, true,
                                                               nextd, log.dig.get() + filled);
            else
                first_pass_scatter<HiT, OutH, DigitCut, true>(c, wk, wk.t_lo.get(), (const HiT*)wk.t_hi.get(), fn, S.lo.get(), (OutH*)S.hi.get(), true, nextd, wire_dig ? S.dig.get() : (u8*)nullptr,
                                                              log.own_window(S.own));
        }
        if (trace) fprintf(stderr, "[cblx grouped] rank %u slice %u: N=%llu own=%llu incoming=%llu filled=%llu\n", me, s, (unsigned long long)N, (unsigned long long)S.own.n,
                           (unsigned long long)incoming, (unsigned long long)filled);
        log.filled += incoming;
        prev_work = std::move(wk);
    }

    // -- senders, nothing on the wire. "replicate": KRN-1 + the first pass over EVERY rank's reads, piece by piece; the pass keeps the records of this
    //    rank's prefix range (they go straight into the log) and drops the others. The own pieces first: the peers' planes are still crossing the links
    //    meanwhile. One rank (`single`): every record is its own.
    void send_local() {
        const CutPlan& M = plan();
        if (rep->src.size() != W) throw Error(CBLX_EINVAL, "replicate: one source per rank (internal error)");
        const u32 Q = std::max(1u, rep->parts), NT = nslices * Q;  // parts per slice, parts per source
        pcnt.assign((size_t)NT * W * 256, 0u);
        pbase.assign((size_t)NT * W, 0u);
        log.alloc();
        u64 over = 0;
        std::vector<DeferredTotals> late;
        for (u32 r = 0; r < W; ++r) if (rep->src[r].cuts.size() != (size_t)NT + 1) throw Error(CBLX_EINVAL, "replicate: slice cuts of a source (internal error)");
        // the own source is planned once (its parts are ranges of the plan) and goes first: the peers' planes are crossing the links meanwhile;
        // then the peers part-major — exchange t carries part t of every peer — each part planned on its own once it has landed
        ChunkPlan PLme;
        std::vector<PlanSlice> pslme(NT);
        BaseView vme = rep->src[me].view;
        const bool own_whole = !rep->per_slice && rep->src[me].nseq != 0;
        if (own_whole) plan_chunks(c, vme, rep->src[me].d_off, rep->src[me].nseq, PLme, nullptr, &rep->src[me].cuts, &pslme);
        std::vector<std::pair<u32, u32>> order;  // (source, part)
        for (u32 t = 0; t < NT; ++t) order.push_back({me, t});
        for (u32 t = 0; t < NT; ++t) for (u32 r = 0; r < W; ++r) if (r != me) order.push_back({r, t});
        for (const auto& rt : order) {
            if (over) break;
            const u32 r = rt.first, t = rt.second, s = t / Q;
            const ReplicaSource& R = rep->src[r];
            if (R.nseq == 0) continue;
            prev_work = FirstPass();
            FirstPass wk;
            const ChunkPlan* pl = &PLme;
            const PlanSlice* part = &pslme[t];
            BaseView vs = vme;
            if (!(r == me && own_whole)) {  // the part is planned once it has landed
                if (rep->ready) rep->ready(t);
                if (r != me) {
                    if (t < rep->part_ready.size() && rep->part_ready[t]) CBLX_HIP(hipStreamWaitEvent(c->stream, rep->part_ready[t], 0));
                    else T.wait();
                }
                if (R.cuts[t + 1] == R.cuts[t]) continue;
                vs = R.view;
                plan_chunks(c, vs, R.d_off + R.cuts[t], R.cuts[t + 1] - R.cuts[t], wk.pl);
                pl = &wk.pl;
                part = nullptr;
            }
            const u64 N = part ? part->k_hi - part->k_lo : pl->n_kmers;
            if (N >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "one slice takes fewer than 2^32-16 words (use more slices)");
            if (!N) continue;
            first_pass_count<C>(c, wk, vs, *pl, N, eh0, part);
            const size_t piece = ((size_t)s * W + r) * Q + (t % Q);
            if (single) {
                // one rank: every record is its own and the pass writes the log directly; the bin counts of the piece stay on the device until
                // the last slice is through (no host round trip between KRN-1 and the first pass: the next slice may be landing)
                if (log.filled + N >= ROUND_LIMIT) { over = 1; break; }
                log.room(log.filled + N);
                pbase[piece] = (u32)log.filled;
                first_pass_scatter<HiT, OutH, DigitCut, false>(c, wk, wk.t_lo.get(), (const HiT*)wk.t_hi.get(), fn, log.lo.get() + log.filled,
                                                               OHS ? (OutH*)(log.hi.get() + log.filled * OHS) : (OutH*)nullptr, true, nextd, log.dig.get() + log.filled);
                late.push_back(DeferredTotals{piece, N, std::move(wk.coltot)});
                log.filled += N;
                prev_work = std::move(wk);
                continue;
            }
            const std::vector<u32> tot = d2h_vec<u32>(c, wk.coltot.get(), 256);
            std::vector<u64> hdr((size_t)W * HDR, 0);
            const OwnShare own = wire_header(M, tot.data(), W, me, N, "piece", hdr.data());
            for (u32 cl = 0; cl < 256; ++cl) pcnt[piece * 256 + cl] = (u32)hdr[(size_t)me * HDR + 1 + cl];
            if (log.filled + own.n >= ROUND_LIMIT) { over = 1; break; }  // (settled with the other ranks below: the job leaves together)
            log.room(log.filled + own.n);
            pbase[piece] = (u32)log.filled;
            // (no send buffer: the pass drops what is not this rank's)
            first_pass_scatter<HiT, OutH, DigitCut, true>(c, wk, wk.t_lo.get(), (const HiT*)wk.t_hi.get(), fn, (u64*)nullptr, (OutH*)nullptr, true, nextd, (u8*)nullptr, log.own_window(own));
            if (trace) fprintf(stderr, "[cblx replicate] rank %u piece (slice %u, source %u, part %u): N=%llu kept=%llu filled=%llu\n", me, s, r, t % Q, (unsigned long long)N,
                               (unsigned long long)own.n, (unsigned long long)log.filled);
            log.filled += own.n;
            prev_work = std::move(wk);
        }
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the own source's plan dies here
        T.wait();
        T.all_reduce_sum_u64(&over, 1);
        if (over) throw Error(CBLX_ERANGE, "a rank's share of the job takes more than one round: use more ranks");
        fold_deferred(c, M, late, "piece", pcnt);  // one rank: the bin counts of every piece, read once the passes are queued
    }

    // prefix window of every group: its cuts (multiples of 64), the range's ends rounded outwards
    u64 group_first_prefix(u32 g) const {
        const CutPlan& M = plan();
        const u64 nprefix = 1ull << P.PB;
        if (g >= NG) return me + 1 < W ? ((u64)bounds[me] + 63) & ~63ull : nprefix;
        if (g == 0) return me ? (u64)bounds[me - 1] & ~63ull : 0ull;
        u32 cl = gc0[g];
        while (cl + 1 < my_cells && M.iv_of[my_lo + cl] == 0xFFFFFFFFu) ++cl;  // (an unused bin number in front of the group's first cell)
        const u32 iv = M.iv_of[my_lo + cl];
        return iv && iv != 0xFFFFFFFFu ? (u64)M.cuts[iv - 1] : 0ull;
    }
    // -- the receiver, group by group behind the wire
    void receive() {
        prev_work = FirstPass();  // (the stream is past the last slice's pass A once the first group is waited for; the workspace is only returned to the pool)
        const u64 filled = log.filled, nwords = std::max<u64>(1, (1ull << P.PB) / 64);
        fin.bv = Buf<u64>(c->pool, nwords);
        CBLX_HIP(hipMemsetAsync(fin.bv.get(), 0, nwords * 8, c->stream));
        fin.a_lo = Buf<u64>(c->pool, filled + 2);
        if (WS) fin.a_hi = Buf<u64>(c->pool, filled + 2);
        else if (OHS) fin_hi_keep = Buf<u64>(c->pool, filled + 2);
        fin_hi = WS ? fin.a_hi.get() : fin_hi_keep.get();
        gN.assign(NG, 0);
        const size_t np = pbase.size();  // nslices * W pieces (times the parts of a slice under "replicate")
        for (size_t p = 0; p < np; ++p)
            for (u32 g = 0; g < NG; ++g)
                for (u32 cl = gc0[g]; cl < gc0[g + 1]; ++cl) gN[g] += pcnt[p * 256 + cl];
        u64 gmax = 0;
        for (u64 x : gN) gmax = std::max(gmax, x);
        Buf<u64> scr_lo(c->pool, gmax + 2), scr_hi(c->pool, OHS ? gmax + 2 : 1);
        Buf<u8> dig2(c->pool, gmax + 64);
        parts.resize(NG);
        gbase.assign(NG + 1, 0);
        for (u32 g = 0; g < NG; ++g) {
            gbase[g + 1] = gbase[g] + gN[g];
            if (g < Gmax && gev.e[g]) CBLX_HIP(hipStreamWaitEvent(c->stream, gev.e[g], 0));
            if (gN[g] == 0) continue;
            GroupRegions R;
            R.log_lo = log.lo.get(); R.log_hi = OHS ? (const void*)log.hi.get() : nullptr;
            R.fin_lo = fin.a_lo.get() + gbase[g]; R.fin_hi = fin_hi ? fin_hi + gbase[g] : nullptr;
            R.scr_lo = scr_lo.get(); R.scr_hi = OHS ? scr_hi.get() : nullptr;
            receive_group(g, R, dig2.get());
        }
        T.wait();
        CBLX_HIP(hipStreamSynchronize(c->stream));
        for (Sent& S : sent) { S.lo.reset(); S.hi.reset(); S.dig.reset(); }
        log.reset();
    }
    // group g's pieces of the log through the LSD passes, its window of the directory and the bucket kernels
    void receive_group(u32 g, const GroupRegions& R, u8* dig2) {
        const CutPlan& M = plan();
        const u64 nprefix = 1ull << P.PB;
        const size_t np = pbase.size();
        // the group's share of every piece: counts per SEGMENT (inside a group a segment occurs in one cell only), first record
        std::vector<u32> cnt_g, pb_g, segp(256, 0xFFFFFFFFu);
        if (fine)  // a bin's records share their prefix bits from the bin's level up: the first prefix of its aligned block
            for (u32 cl = gc0[g]; cl < gc0[g + 1]; ++cl) {
                const u32 bin = my_lo + cl, iv = M.iv_of[bin];
                if (iv == 0xFFFFFFFFu) continue;
                // (the all-ones bin: the block of 2^sort_bits prefixes that ends at 2^PREFIX_BITS — its records OR their low bits back in and land
                // on the all-ones prefix; with the all-ones prefix ITSELF as the base every row of k_dir_gather's table for this segment
                // mapped to that one prefix, one of them with the real start and the others with EMPTY, unordered)
                const u32 sbg = FM.sort_bits[me][g];
                segp[FM.seg_of[bin]] = bin == 255 ? (u32)((((1ull << P.PB) - 1) >> sbg) << sbg) : (FM.first[iv] >> FM.level[iv]) << FM.level[iv];
            }
        group_piece_table((fine ? FM.seg_of : M.v_of) + my_lo, gc0[g], gc0[g + 1], pcnt, pbase, cnt_g, pb_g);
        PieceInput pin;
        pin.np = (u32)np; pin.cnt = cnt_g.data(); pin.pbase = pb_g.data();
        if (wire_dig) { pin.dig_in = log.dig.get(); pin.dig_out = dig2; }  // (else: the first histogram reads the records, the later passes' digits go to a buffer of the pass's own)
        if (fine) { pin.sort_bits = FM.sort_bits[me][g]; pin.seg_prefix = segp.data(); }
        DirWindow win;
        win.w_lo = (u32)group_first_prefix(g);
        u64 whi = group_first_prefix(g + 1);
        if (fine && whi > (nprefix >> 1) && win.w_lo < (nprefix >> 1)) {
            // FINE bins: no necklace prefix lies in the upper half of the prefix space except the all-ones word's (bin 255): a group that
            // reaches up there and holds no such word ends its directory window at the half (the dense directory costs a pass over the window)
            u64 ones = 0;
            if (my_lo + my_cells == 256) for (size_t p = 0; p < np; ++p) ones += pcnt[p * 256 + (255 - my_lo)];
            if (!ones) whi = nprefix >> 1;
        }
        win.w_hi = (u32)std::min<u64>(whi, 0xFFFFFFC0ull);
        win.bv = fin.bv.get();
        if (trace) fprintf(stderr, "[cblx grouped] rank %u group %u: %llu words, prefixes [%u, %u), cells [%u, %u), %u bits sorted behind the first pass\n", me, g, (unsigned long long)gN[g], win.w_lo, win.w_hi,
                           gc0[g], gc0[g + 1], pin.sort_bits ? pin.sort_bits : RB);
        pipeline_group<C>(c, R, pin, gN[g], win, parts[g]);
        ++cm->groups_used;
        if (pin.sort_bits == FINE_LEVEL) ++cm->groups_fine;
    }

    // -- one index out of the groups: tables concatenated (starts made absolute), rank directory over the whole bitvector
    void assemble() {
        const u64 filled = log.filled, nwords = std::max<u64>(1, (1ull << P.PB) / 64);
        if (filled) {
            u64 nb = 0;
            for (const Resident& r : parts) { nb += r.nb; fin.count += r.count; }
            fin.nb = nb;
            fin.prefix = Buf<u32>(c->pool, nb + 1); fin.start = Buf<u64>(c->pool, nb + 1);
            fin.cnt = Buf<u32>(c->pool, nb + 1); fin.kind = Buf<u8>(c->pool, nb + 1);
            u64 at = 0;
            for (u32 g = 0; g < NG; ++g) {
                const Resident& r = parts[g];
                if (!r.nb) continue;
                CBLX_HIP(hipMemcpyAsync(fin.prefix.get() + at, r.prefix.get(), r.nb * 4, hipMemcpyDeviceToDevice, c->stream));
                CBLX_HIP(hipMemcpyAsync(fin.start.get() + at, r.start.get(), r.nb * 8, hipMemcpyDeviceToDevice, c->stream));
                CBLX_HIP(hipMemcpyAsync(fin.cnt.get() + at, r.cnt.get(), r.nb * 4, hipMemcpyDeviceToDevice, c->stream));
                CBLX_HIP(hipMemcpyAsync(fin.kind.get() + at, r.kind.get(), r.nb, hipMemcpyDeviceToDevice, c->stream));
                if (gbase[g]) hipLaunchKernelGGL(k_add_u64, grid1(r.nb, 256), dim3(256), 0, c->stream, fin.start.get() + at, r.nb, gbase[g]);
                at += r.nb;
            }
            hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, fin.start.get() + nb, filled);
            Buf<u32> popc(c->pool, nwords);
            fin.rank_dir = Buf<u64>(c->pool, nwords + 1);
            hipLaunchKernelGGL(k_setop_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, (const u64*)fin.bv.get(), (const u64*)fin.bv.get(), SETOP_OR, fin.bv.get(), popc.get());
            const u64 nb2 = exclusive_scan<u64>(c, popc.get(), nwords, fin.rank_dir.get());
            CBLX_HIP(hipGetLastError());
            if (nb2 != nb) throw Error(CBLX_EDEVICE, "grouped receiver: the groups hold " + std::to_string(nb) + " buckets, the bitvector " + std::to_string(nb2) + " (internal error)");
            CBLX_HIP(hipStreamSynchronize(c->stream));
            parts.clear();
            c->res = std::move(fin);
            c->kmers_inserted += filled;
        }
        CBLX_HIP(hipStreamSynchronize(c->stream));
    }
};
template <typename C>
bool sharded_insert_grouped(cblx_ctx* c, cblx_comm* cm, const u8* d_bases, const u64* d_offsets, u64 n, const u64* cuts, u32 nslices, const u32* bounds, bool single = false,
                            const Replica* rep = nullptr) {
    GroupedInsert<C> J{c, cm, d_bases, d_offsets, n, cuts, nslices, bounds, single, rep};
    if (!J.resolve()) return false;
    if (rep) J.send_local(); else J.send_wire();
    J.receive();
    J.assemble();
    return true;
}

// ---- protocol "replicate" (round 6): ship READS, not words -----------------------------------------------------------------------------
// Between 2 - 4 GPUs every pair shares ONE xGMI link, and the words of the other protocols put 5 - 8 bytes per k-mer on it: at cfg 3 and 55 GB/s
// per link two ranks take 101 ms per step ("sorted"; 127 "bins") where ONE GPU builds the same reads in 39 (profiles/r05_wire_emulated.md). The
// k-mer -> word transform is a pure function of the bases, and the bases are 0.3 bytes per k-mer as bit planes (3 bits per base,
// 150 / 120 bases per k-mer): every rank packs ITS reads into planes on the device (k_pack_planes), the planes and the read offsets are
// all-gathered, and every rank runs KRN-1 and the first partition pass over ALL ranks' reads, keeping the words of its own prefix range
// (k_radix_scatter drops the others where it would have sent them) — W encodes per rank instead of one, nothing else added, and the job's stream
// order (slice-major, rank-minor) holds by construction: the pieces are the same (slice, source) pieces the "bins" receiver sees, made locally.
// The receiver steps (groups, FINE bins, directory windows, bucket kernels) are sharded_insert_grouped's own.
template <typename C>
bool sharded_insert_replicate(cblx_ctx* c, cblx_comm* cm, const u8* d_bases, const u64* d_offsets, u64 n, const u64* cuts, u32 nslices, const u32* bounds) {
    Transport& T = *cm->t;
    const u32 W = T.world, me = T.rank;
    if (W < 2 || nslices == 0) return false;
    check_aligned16(d_bases, "d_bases");
    check_slice_cuts(cuts, nslices, n);
    const u64 n0 = cuts[0], n1 = cuts[nslices], nseq = n1 - n0;
    // The planes cross the links in PARTS (two per call at least: a one-slice call is cut in halves of its reads) so that a peer's first part can be
    // transformed while its later ones are still on the wire; parts cut the (slice, source) pieces, they do not reorder them. (Every part of every
    // peer is planned on its own — 0.4 ms of host round trips each: four parts were measured too and cost what they hid at 55 GB/s per link.)
    const u32 Q = std::max(1u, 2u / nslices), NT = nslices * Q;
    std::vector<u64> xcuts(NT + 1), ox(NT + 1, 0);  // sequence index (relative to n0) and base offset at every part boundary
    for (u32 s = 0; s < nslices; ++s)
        for (u32 q = 0; q < Q; ++q) xcuts[s * Q + q] = cuts[s] - n0 + (cuts[s + 1] - cuts[s]) * q / Q;
    xcuts[NT] = nseq;
    if (nseq) {
        for (u32 t = 0; t <= NT; ++t) ox[t] = (t && xcuts[t] == xcuts[t - 1]) ? ox[t - 1] : d2h<u64>(c, d_offsets + n0 + xcuts[t]);
        for (u32 t = 0; t < NT; ++t) (void)offsets_span(ox[t], ox[t + 1]);
    }
    const u64 first = ox[0], last = ox[NT];
    const u64 g0 = first >> 4, g1 = nseq ? (last + 15) >> 4 : g0, ng = g1 - g0;
    // -- what every rank holds: sequences, part boundaries (sequence index and base offset)
    const size_t per = 1 + 2 * ((size_t)NT + 1);
    std::vector<u64> send(per * W), recv(per * W);
    for (u32 d = 0; d < W; ++d) {
        u64* h = send.data() + d * per;
        h[0] = nseq;
        for (u32 t = 0; t <= NT; ++t) { h[1 + t] = xcuts[t]; h[2 + NT + t] = ox[t]; }
    }
    T.all_to_all_u64(send.data(), recv.data(), per);
    auto hdr_cut = [&](u32 r, u32 t) { return recv[r * per + 1 + t]; };
    auto hdr_off = [&](u32 r, u32 t) { return recv[r * per + 2 + NT + t]; };
    auto ga_of = [&](u32 r, u32 t) { return hdr_off(r, t) >> 4; };                                           // first plane group of part t of rank r
    auto gb_of = [&](u32 r, u32 t) { return recv[r * per] ? (hdr_off(r, t + 1) + 15) >> 4 : ga_of(r, t); };  // one past its last
    // -- own planes, then the all-gather of planes and offsets, part by part (the own pieces are transformed under it)
    Buf<u32> my_codes(c->pool, ng + 4);
    Buf<u16> my_valid(c->pool, ng + 4);
    if (ng) hipLaunchKernelGGL(k_pack_planes, grid1(ng, 256), dim3(256), 0, c->stream, d_bases, g0, g1, last, my_codes.get(), my_valid.get());
    CBLX_HIP(hipGetLastError());
    std::vector<u64> gro(W + 1, 0), sqo(W + 1, 0);  // plane groups / offset words in front of every peer's share of the gather buffers
    for (u32 r = 0; r < W; ++r) {
        for (u32 t = 0; t < NT; ++t) if (hdr_cut(r, t + 1) < hdr_cut(r, t) || hdr_off(r, t + 1) < hdr_off(r, t)) throw Error(CBLX_EDEVICE, "replicate: a rank announced part boundaries out of order (transport error)");
        if (hdr_cut(r, NT) != recv[r * per]) throw Error(CBLX_EDEVICE, "replicate: a rank's parts do not add up to its reads (transport error)");
        const u64 ngr = recv[r * per] ? gb_of(r, NT - 1) - ga_of(r, 0) : 0;
        gro[r + 1] = gro[r] + (r == me ? 0 : ngr + 4);  // (+ slack: the tile loads of KRN-1 read a few words ahead)
        sqo[r + 1] = sqo[r] + (r == me ? 0 : recv[r * per] + 1);
    }
    Buf<u32> all_codes(c->pool, gro[W] + 4);
    Buf<u16> all_valid(c->pool, gro[W] + 4);
    Buf<u64> all_off(c->pool, sqo[W] + 2);
    CBLX_HIP(hipMemsetAsync(all_codes.get(), 0, (gro[W] + 4) * 4, c->stream));
    CBLX_HIP(hipMemsetAsync(all_valid.get(), 0, (gro[W] + 4) * 2, c->stream));
    EventOwner ev;
    ev.e.assign(NT, nullptr);
    Drain drain{&T};
    for (u32 t = 0; t < NT; ++t) {
        auto planes = [&](const void* src, void* dst, size_t es) {
            Transport::Item it{(const u8*)src, (u8*)dst, std::vector<u64>(W, 0), std::vector<u64>(W, 0), std::vector<u64>(W, 0), std::vector<u64>(W, 0)};
            for (u32 r = 0; r < W; ++r) {
                if (r == me) continue;
                it.s_off[r] = (ga_of(me, t) - ga_of(me, 0)) * es;
                it.s_len[r] = (gb_of(me, t) - ga_of(me, t)) * es;
                it.r_off[r] = (gro[r] + ga_of(r, t) - ga_of(r, 0)) * es;
                it.r_len[r] = (gb_of(r, t) - ga_of(r, t)) * es;
            }
            return it;
        };
        std::vector<Transport::Item> items;
        items.push_back(planes(my_codes.get(), all_codes.get(), 4));
        items.push_back(planes(my_valid.get(), all_valid.get(), 2));
        if (t == 0) {  // every read offset rides with the first part
            Transport::Item it{(const u8*)(d_offsets + n0), (u8*)all_off.get(), std::vector<u64>(W, 0), std::vector<u64>(W, 0), std::vector<u64>(W, 0), std::vector<u64>(W, 0)};
            for (u32 r = 0; r < W; ++r) {
                if (r == me) continue;
                it.s_len[r] = nseq ? (nseq + 1) * 8 : 0;
                it.r_off[r] = sqo[r] * 8;
                it.r_len[r] = recv[r * per] ? (recv[r * per] + 1) * 8 : 0;
            }
            items.push_back(std::move(it));
        }
        T.exchange_items(items, c->stream);
        CBLX_HIP(hipEventCreateWithFlags(&ev.e[t], hipEventDisableTiming));
        T.record(ev.e[t], c->stream);
    }
    Replica rep;
    rep.src.resize(W);
    rep.parts = Q;
    rep.part_ready = ev.e;
    for (u32 r = 0; r < W; ++r) {
        ReplicaSource& R = rep.src[r];
        R.nseq = recv[r * per];
        for (u32 t = 0; t <= NT; ++t) R.cuts.push_back(hdr_cut(r, t));
        if (r == me) { R.view = ascii_view(d_bases); R.d_off = d_offsets + n0; }
        else {  // planes indexed by the SENDER's base positions: group g of the sender is word g - (its first group) of its share
            R.view = BaseView{nullptr, all_codes.get() + gro[r] - ga_of(r, 0), all_valid.get() + gro[r] - ga_of(r, 0)};
            R.d_off = all_off.get() + sqo[r];
        }
    }
    const bool done = sharded_insert_grouped<C>(c, cm, d_bases, d_offsets, n, cuts, nslices, bounds, false, &rep);
    T.wait();
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the gather buffers die here
    return done;
}

// one rank's FINE plan: the one "group cut" below which the bins are blocks of 2^16 prefixes (insert_device_fine; a one-rank communicator)
inline u32 fine_single_cut(u32 PB) { return std::min<u32>(245u << FINE_LEVEL, (1u << (PB - 1)) - (1u << FINE_LEVEL)); }
template <typename C>
void sharded_insert(cblx_ctx* c, cblx_comm* cm, const u8* d_bases, const u64* d_offsets, u64 n, const u64* cuts, u32 nslices, u32* bounds, int* bounds_valid) {
    Transport& T = *cm->t;
    T.begin_job();
    if (nslices && !*bounds_valid) {
        check_slice_cuts(cuts, 1, n);
        std::vector<u64> hist;
        const u32 asked = cm->protocol == CBLX_PROTO_AUTO ? auto_protocol(T.world) : cm->protocol;
        const bool want_bins = asked == CBLX_PROTO_BINS || asked == CBLX_PROTO_REPLICATE;
        const u32 G = recv_groups_wanted(cm);
        choose_bounds_from_slice<C>(c, T, d_bases, d_offsets + cuts[0], cuts[1] - cuts[0], bounds, &hist, (want_bins && G >= 2) ? G : 0u);
        *bounds_valid = 1;
        if (T.world > 1) {  // the group cuts of the grouped receiver come from the same histogram
            cm->g_cuts = choose_group_cuts(hist, bounds, T.world, recv_groups_wanted(cm), c->P.PB);
            cm->g_bounds.assign(bounds, bounds + (T.world - 1));
        }
    }
    cm->groups_used = 0;
    cm->groups_fine = 0;
    u32 proto = cm->protocol == CBLX_PROTO_AUTO ? auto_protocol(T.world) : cm->protocol;
    if ((proto == CBLX_PROTO_BINS || proto == CBLX_PROTO_REPLICATE) && !bins_protocol_fits(c->P, bounds, T.world)) proto = CBLX_PROTO_SORTED;
    if (proto == CBLX_PROTO_REPLICATE) {
        // (every term of the decision inside is replicated: the ranks take the fallback together)
        cm->protocol_used = CBLX_PROTO_REPLICATE;
        if (T.world >= 2 && sharded_insert_replicate<C>(c, cm, d_bases, d_offsets, n, cuts, nslices, bounds)) return;
        proto = CBLX_PROTO_BINS;  // a non-empty index, a plan the cuts refuse, one rank: the records cross the wire as before
    }
    cm->protocol_used = proto;
    if (proto == CBLX_PROTO_BINS) {
        if (T.world == 1 && c->P.PB > 24 && c->res.count == 0) {
            // a one-rank group at PREFIX_BITS > 24: the FINE-bins build of insert_device_fine on this communicator (its slices as given)
            std::vector<u32> keep = std::move(cm->g_cuts);
            cm->g_cuts.assign(1, fine_single_cut(c->P.PB));
            bool done = false;
            try { done = sharded_insert_grouped<C>(c, cm, d_bases, d_offsets, n, cuts, nslices, bounds, true); } catch (...) { cm->g_cuts = std::move(keep); throw; }
            cm->g_cuts = std::move(keep);
            if (done) { ++c->fine_builds; return; }
        }
        if (sharded_insert_grouped<C>(c, cm, d_bases, d_offsets, n, cuts, nslices, bounds)) return;
        sharded_insert_bins<C>(c, T, ascii_view(d_bases), d_offsets, n, cuts, nslices, bounds, [](u32) {});
    }
    else
        sharded_insert_sorted<C>(c, T, d_bases, d_offsets, n, cuts, nslices, bounds, bounds_valid);
}

// ---- one GPU, a batch that is still arriving: the same slice-by-slice path on a one-rank "group" ---------------------------------
struct LocalTransport : Transport {
    LocalTransport() { rank = 0; world = 1; }
    void all_reduce_sum_u64(u64*, size_t) override {}
    void all_to_all_u64(const u64* send, u64* recv, size_t per) override { std::memcpy(recv, send, per * 8); }
    void exchange(const u8*, const u64*, u8*, const u64*, hipStream_t) override {}
    void wait() override {}
    void exchange_items(const std::vector<Item>&, hipStream_t) override {}
};
// the one-rank communicator of the FINE-bins build: no wire, two "groups" cut at fine_single_cut
inline void fine_local_comm(cblx_comm& cm, u32 PB) {
    cm.t.reset(new LocalTransport());
    cm.recv_groups = 2;
    cm.g_cuts.assign(1, fine_single_cut(PB));
}
// ---- one GPU, PREFIX_BITS > 24, an empty index: the build on FINE bins --------------------------------------------------------------
// The plain build sorts 24 prefix bits in three passes and finishes the last PREFIX_BITS - 24 run by run (k_prefix_split): four trips
// of every record through HBM. Here the first pass runs on the FINE bins of the grouped receiver (cuts.hpp: make_fine_plan) with ONE
// rank and TWO "groups": the prefixes below 245 * 2^16 — where nearly nine tenths of the necklace prefixes of random reads lie — in
// aligned blocks of 2^16 prefixes, whose records need 16 more bits sorted (two passes), and the rest in blocks of 2^24 (three passes of
// 8 bits). No sampling: the cut is fixed, and a batch whose words all lie above it simply takes three passes behind the first, as the
// plain build does. Same index (tests run every PREFIX_BITS > 24 shape through both routes).
bool insert_device_fine(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq) {
    if (!fine_bins_enabled() || c->P.PB <= 24 || nseq == 0 || c->res.count != 0) return false;
    check_aligned16(d_bases, "d_bases");
    cblx_comm cm;
    fine_local_comm(cm, c->P.PB);
    const u64 cuts[2] = {0, nseq};
    bool done = false;
    dispatch(c->P, [&](auto cfg) { done = sharded_insert_grouped<decltype(cfg)>(c, &cm, d_bases, d_offsets, nseq, cuts, 1, nullptr, true); });
    if (done) ++c->fine_builds;
    return done;
}
}  // namespace
