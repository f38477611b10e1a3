// list.hpp — reading the index out, on the host: where every bucket begins in the iteration order (iteration_offsets), a range of that order as packed
// k-mers or as text lines (export_range_launch, range_clamp), and `cbl list` — a text streamed from the device to a file descriptor through two pinned
// buffers and a writer thread (stream_chunks_to_fd, list_to_fd). Kernels: kernels_list.hpp. Included by cblx.cpp only (through graph.hpp, whose passes
// export their k-mers here).
#pragma once
#include "ingest.hpp"
#include "kernels_list.hpp"

namespace {

// res_off[nb + 1]: where every bucket begins in the iteration order, and the total behind the last one
u64 iteration_offsets(cblx_ctx* c, Buf<u64>& res_off) {
    const Resident& r = c->res;
    res_off = Buf<u64>(c->pool, r.nb + 1);
    const u64 tot = exclusive_scan<u64>(c, r.cnt.get(), r.nb, res_off.get());
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, res_off.get() + r.nb, tot);
    CBLX_HIP(hipGetLastError());
    return tot;
}
// elements [first, first + n) of the iteration order (n != 0, inside the index) to device arrays, from their index 0; asynchronous on the ctx's stream.
// d_text != null: lines (16-byte aligned); else packed k-mers, d_hi may be null.
void export_range_launch(cblx_ctx* c, const u64* res_off, u64 first, u64 n, u64* d_lo, u64* d_hi, u8* d_text) {
    const Resident& r = c->res;
    const u64 LINE = c->P.K + 1, STEP = 1ull << 31;  // one launch addresses fewer than 2^32 work items; a multiple of LIST_THREADS keeps every text launch 16-byte aligned
    const bool ws = c->P.wide_suffix();
    for (u64 o = 0; o < n; o += STEP) {
        const u64 m = std::min<u64>(STEP, n - o);
        const dim3 grid = grid1(m, LIST_THREADS);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, grid, dim3(LIST_THREADS), 0, c->stream, first + o, m, r.nb, res_off, r.prefix.get(), r.start.get(), r.a_lo.get(),
                               ws ? r.a_hi.get() : (const u64*)nullptr, c->P, d_text ? (u64*)nullptr : d_lo + o, (d_text || !d_hi) ? (u64*)nullptr : d_hi + o,
                               d_text ? d_text + o * LINE : (u8*)nullptr);
        };
        if (d_text) { if (ws) go(k_export_range<true, true>); else go(k_export_range<true, false>); }
        else { if (ws) go(k_export_range<false, true>); else go(k_export_range<false, false>); }
    }
    CBLX_HIP(hipGetLastError());
}
// the checks the range calls share: *m = min(n, count - first)
void range_clamp(cblx_ctx* c, u64 first, u64 n, u64* m) {
    flush(c);
    if (first > c->res.count) throw Error(CBLX_EINVAL, "first = " + std::to_string(first) + " is past the end: the index holds " + std::to_string(c->res.count) + " k-mers");
    *m = std::min<u64>(n, c->res.count - first);
}

// `cbl list`: the lines of the whole index to a file descriptor, chunk by chunk. Two device buffers and two pinned ones: while the device emits
// chunk i, chunk i - 1 crosses to its pinned buffer and a writer thread hands chunk i - 2 to write(), in order.
static const u64 LIST_CHUNK_DEFAULT = 1ull << 21;
// The stream itself: `total` bytes (not 0) in chunks of `cbytes`. emit(i, len) queues on the ctx's stream whatever makes chunk i and returns where its
// len bytes will be on the device; what it returned for chunk i - 2 is free again when it is called for chunk i. `what` names the text in the message
// of a failed write.
template <typename Emit> void stream_chunks_to_fd(cblx_ctx* c, int fd, u64 total, u64 cbytes, const char* what, Emit&& emit) {
    const u64 nch = ceil_div(total, cbytes);
    const u8* src_dev[2] = {nullptr, nullptr};
    struct Pinned {
        u8* p[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Pinned() { for (int i = 0; i < 2; ++i) { if (p[i]) (void)hipHostFree(p[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); } }
    } pin;
    for (int i = 0; i < (nch > 1 ? 2 : 1); ++i) CBLX_HIP(hipHostMalloc((void**)&pin.p[i], cbytes, hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) CBLX_HIP(hipEventCreateWithFlags(&pin.ev[i], hipEventDisableTiming));
    struct Drain {  // on any way out no emitter is still writing into a buffer that goes back to the pool
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{c->stream};
    // the writer: chunks [0, handed) may be written, `written` are done; it stops at the first error
    struct Writer {
        std::mutex mu;
        std::condition_variable cv;
        u64 handed = 0, written = 0;
        bool quit = false;
        int err = 0;  // errno of a failed write, EIO for one that wrote nothing
        std::thread th;
        ~Writer() { { std::lock_guard<std::mutex> g(mu); quit = true; } cv.notify_all(); if (th.joinable()) th.join(); }
    } wr;
    auto chunk_len = [&](u64 i) { return std::min<u64>(cbytes, total - i * cbytes); };
    wr.th = std::thread([&] {
        for (u64 i = 0;; ++i) {
            {
                std::unique_lock<std::mutex> g(wr.mu);
                wr.cv.wait(g, [&] { return wr.quit || wr.handed > i; });
                if (wr.handed <= i) return;
            }
            const u8* src = pin.p[i & 1];
            u64 left = chunk_len(i);
            int err = 0;
            while (left) {
                const ssize_t k = ::write(fd, src, left);
                if (k < 0 && errno == EINTR) continue;
                if (k <= 0) { err = k < 0 ? errno : EIO; break; }
                src += k; left -= (u64)k;
            }
            std::lock_guard<std::mutex> g(wr.mu);
            if (err) { wr.err = err; wr.cv.notify_all(); return; }
            wr.written = i + 1;
            wr.cv.notify_all();
        }
    });
    auto fail_if_bad = [&] { if (wr.err) throw Error(CBLX_EINVAL, std::string("Failed to write the ") + what + ": " + std::strerror(wr.err)); };
    for (u64 i = 0; i <= nch; ++i) {
        if (i < nch) {  // chunk i - 2 was downloaded in the previous round
            src_dev[i & 1] = emit(i, chunk_len(i));
            CBLX_HIP(hipEventRecord(pin.ev[i & 1], c->stream));
        }
        if (i >= 1) {
            const u64 j = i - 1;
            CBLX_HIP(hipEventSynchronize(pin.ev[j & 1]));
            {
                std::unique_lock<std::mutex> g(wr.mu);  // the pinned buffer of chunk j still holds chunk j - 2 until that is written
                wr.cv.wait(g, [&] { return wr.err || wr.written + 2 > j; });
                fail_if_bad();
            }
            xfer(c).d2h_copy(pin.p[j & 1], src_dev[j & 1], chunk_len(j));
            { std::lock_guard<std::mutex> g(wr.mu); wr.handed = j + 1; }
            wr.cv.notify_all();
        }
    }
    std::unique_lock<std::mutex> g(wr.mu);
    wr.cv.wait(g, [&] { return wr.err || wr.written == nch; });
    fail_if_bad();
}
void list_to_fd(cblx_ctx* c, int fd, u64 chunk, u64* n_kmers) {
    flush(c);
    const Resident& r = c->res;
    if (n_kmers) *n_kmers = r.count;
    if (r.count == 0) return;
    if (chunk == 0) chunk = LIST_CHUNK_DEFAULT;
    chunk = std::min<u64>(chunk, r.count);
    const u64 LINE = c->P.K + 1, cbytes = chunk * LINE, nch = ceil_div(r.count, chunk);
    Buf<u64> res_off;
    iteration_offsets(c, res_off);
    Buf<u8> dev[2] = {Buf<u8>(c->pool, cbytes), Buf<u8>(c->pool, nch > 1 ? cbytes : 1)};
    stream_chunks_to_fd(c, fd, r.count * LINE, cbytes, "list", [&](u64 i, u64) -> const u8* {
        export_range_launch(c, res_off.get(), i * chunk, std::min<u64>(chunk, r.count - i * chunk), nullptr, nullptr, dev[i & 1].get());
        return dev[i & 1].get();
    });
}

}  // namespace
