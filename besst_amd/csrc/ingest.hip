// BAM file -> resident records: the host-decode ingest (besst_ctx_push_bam), the device ingest (besst_ctx_push_bam_device and
// its part and slice forms) over the kernels of bgzf_gpu.hip, the pinned staging both forms share, and the inflate test hook.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "context.h"
#include "ingest_layout_core.h"

using namespace besst;

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// Work nobody waits for (freeing an ingest's device scratch): threads that are joined when the next one starts, when a
// context is destroyed and by besst_release_cached_memory() - never left running behind the library's last call.
struct Background {
    std::mutex mu;
    std::vector<std::thread> threads;
    ~Background() {                                          // (process exit with a context never destroyed: let them go)
        for (std::thread& t : threads)
            if (t.joinable()) t.detach();
    }
    void join_all() {
        std::vector<std::thread> mine;
        {
            std::lock_guard<std::mutex> g(mu);
            mine.swap(threads);
        }
        for (std::thread& t : mine)
            if (t.joinable()) t.join();
    }
    template <class F>
    void run(F f) {
        join_all();
        std::lock_guard<std::mutex> g(mu);
        threads.emplace_back(std::move(f));
    }
};
Background g_background;

// ---- pinned staging buffers are kept -------------------------------------------------------------------------------
// Pinning and unpinning host memory costs ~90 ms per GB on the bench host - 47 of the 220 ms an ingest of a 40 M-record
// file took, most of it the release at the end of the call.  The staging buffers of the two ingest forms therefore come
// from a process-wide pool and go back to it: a later call (the next library's file, the other form, the next context)
// finds them pinned.  The pool holds at most kPinnedKeep bytes (what comes back beyond that is freed), is never freed at
// exit (the runtime may be gone by then), and besst_release_cached_memory() empties it.
constexpr size_t kPinnedKeep = (size_t)1 << 30;
struct PinnedPool {
    struct Entry { void* p; size_t bytes; bool busy; };
    std::mutex mu;
    std::vector<Entry> all;
    void* acquire(size_t bytes) {
        {
            std::lock_guard<std::mutex> g(mu);
            Entry* best = nullptr;
            for (Entry& e : all)
                if (!e.busy && e.bytes >= bytes && e.bytes <= bytes + bytes / 2 + ((size_t)1 << 20) && (!best || e.bytes < best->bytes)) best = &e;
            if (best) { best->busy = true; return best->p; }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
            trim(0);                                          // (what is cached may be what is missing)
            if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        }
        std::lock_guard<std::mutex> g(mu);
        all.push_back(Entry{p, bytes, true});
        return p;
    }
    void give_back(void* p) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(mu);
            for (Entry& e : all)
                if (e.p == p) e.busy = false;
        }
        trim(kPinnedKeep);
    }
    // free idle buffers, largest first, until at most `keep` idle bytes are left
    void trim(size_t keep) {
        for (;;) {
            void* victim = nullptr;
            {
                std::lock_guard<std::mutex> g(mu);
                size_t idle = 0;
                size_t at = all.size();
                for (size_t i = 0; i < all.size(); ++i)
                    if (!all[i].busy) {
                        idle += all[i].bytes;
                        if (at == all.size() || all[i].bytes > all[at].bytes) at = i;
                    }
                if (idle <= keep || at == all.size()) return;
                victim = all[at].p;
                all.erase(all.begin() + (long)at);
            }
            (void)hipHostFree(victim);
        }
    }
};
PinnedPool g_pinned;

// Room in the record columns for the whole file at the rate so far (+ 6 %), at least for the chunk at hand: `pushed` records
// of this call, that chunk's included, came from `read_bytes` of the `span_bytes` it will read; `resident` were there before.
int64_t column_room(int64_t resident, int64_t pushed, int64_t read_bytes, int64_t span_bytes) {
    const int64_t need = resident + pushed;
    int64_t want = need;
    if (read_bytes > 0 && read_bytes < span_bytes)
        want = resident + (int64_t)((double)pushed * ((double)span_bytes / (double)read_bytes) * 1.06) + 4096;
    if (want < need) want = need;
    if (want >= ((int64_t)1 << 32)) want = ((int64_t)1 << 32) - 1;
    return want;
}

// ---- the layout a device ingest leaves beside the columns: its buffers ---------------------------------------------------
// A plane / the offsets with room for `want` elements: the first `keep` carried over, everything behind them zero (the
// planes are ORed into).
template <class T>
int regrow_zeroed(besst_ctx* c, DevBuf<T>& buf, size_t keep, size_t want) {
    if (want <= buf.cap) return BESST_OK;
    DevBuf<T> bigger;
    int rc = bigger.ensure(want);
    if (rc) return rc;
    if (keep > buf.cap) keep = buf.cap;
    hipError_t e = hipMemsetAsync(bigger.p, 0, bigger.cap * sizeof(T), c->stream);
    if (e == hipSuccess && keep) e = hipMemcpyAsync(bigger.p, buf.p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        bigger.release();
        set_error("push_bam_device: %s", hipGetErrorString(e));
        return BESST_ERR_HIP;
    }
    buf.release();
    buf = bigger;
    return BESST_OK;
}

// the context's stream descriptor points at the buffers where they lie now (counts and n_refs stay)
void point_stream(besst_ctx* c) {
    const size_t cap = (size_t)c->cs_cap_entries;
    char* e = reinterpret_cast<char*>(c->cs_entries.p);
    c->cs.offsets = c->cs_off.p;
    c->cs.set_bits = c->cs_set.p;
    c->cs.tid = e; c->cs.mtid = e + cap * 4; c->cs.pos = e + cap * 8; c->cs.mpos = e + cap * 12;
    c->cs.flag_qlen = e + cap * 16; c->cs.mapq = e + cap * 20;
}

// The six entry columns carved anew for `cap` entries each (a multiple of 64), the first `valid` entries of every column
// carried over to the new stride.
int carve_entries(besst_ctx* c, int64_t cap, int64_t valid) {
    uint8_t* p = nullptr;
    if (hipMalloc((void**)&p, (size_t)cap * 21) != hipSuccess) {
        set_error("push_bam_device: cannot allocate %zu bytes for the candidate entries", (size_t)cap * 21);
        return BESST_ERR_NOMEM;
    }
    const size_t old = (size_t)c->cs_cap_entries;
    static const size_t at[6] = {0, 4, 8, 12, 16, 20}, width[6] = {4, 4, 4, 4, 4, 1};
    hipError_t e = hipSuccess;
    if (valid > (int64_t)old) valid = (int64_t)old;
    for (int k = 0; k < 6 && e == hipSuccess && valid > 0; ++k)
        e = hipMemcpyAsync(p + (size_t)cap * at[k], c->cs_entries.p + old * at[k], (size_t)valid * width[k], hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        set_error("push_bam_device: %s", hipGetErrorString(e));
        return BESST_ERR_HIP;
    }
    c->cs_entries.release();
    c->cs_entries.p = p;
    c->cs_entries.cap = (size_t)cap * 21;
    c->cs_cap_entries = cap;
    return BESST_OK;
}

}  // namespace

void besst::ingest_join_background() { g_background.join_all(); }

extern "C" void besst_release_cached_memory(void) {
    g_background.join_all();
    g_pinned.trim(0);
}

// BAM file -> resident records, streamed: chunks of the file are inflated and decoded by the reader's host threads into
// one of two sets of PINNED staging columns while the previous chunk's eight asynchronous copies are still on their way
// to HBM - decode and upload overlap, no pageable copy, no host-side concatenation of the whole stream.
extern "C" int besst_ctx_push_bam(besst_ctx* c, besst_bam* bam, int64_t chunk_records, int64_t head_records, int32_t* head_rlen,
                                  int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats) {
    BESST_REQUIRE(c && bam, "push_bam: null context or reader");
    BESST_REQUIRE(head_records >= 0 && (head_records == 0 || (head_rlen && head_alen && head_qlen)), "push_bam: head buffers missing");
    if (chunk_records <= 0) chunk_records = (int64_t)4 << 20;
    if (chunk_records < 1024) chunk_records = 1024;
    int rc = use_device(c);
    if (rc) return rc;
    const auto t_start = Clock::now();
    struct Slot {
        int32_t *tid = nullptr, *mtid = nullptr, *pos = nullptr, *mpos = nullptr, *tlen = nullptr;
        uint16_t *flag = nullptr, *qlen = nullptr;
        uint8_t* mapq = nullptr;
        hipEvent_t done = nullptr;
        bool busy = false;
    } slot[2];
    std::vector<int32_t> rlen((size_t)chunk_records), alen((size_t)chunk_records);
    auto release = [&]() {
        for (Slot& sl : slot) {
            void* ptrs[8] = {sl.tid, sl.mtid, sl.pos, sl.mpos, sl.tlen, sl.flag, sl.qlen, sl.mapq};
            for (void* q : ptrs) g_pinned.give_back(q);
            if (sl.done) (void)hipEventDestroy(sl.done);
            sl = Slot();
        }
    };
    auto pinned = [&](void** out, size_t bytes) { return (*out = g_pinned.acquire(bytes)) != nullptr; };
    bool ok = true;
    for (Slot& sl : slot) {
        const size_t m = (size_t)chunk_records;
        ok = ok && pinned((void**)&sl.tid, m * 4) && pinned((void**)&sl.mtid, m * 4) && pinned((void**)&sl.pos, m * 4) &&
             pinned((void**)&sl.mpos, m * 4) && pinned((void**)&sl.tlen, m * 4) && pinned((void**)&sl.flag, m * 2) &&
             pinned((void**)&sl.qlen, m * 2) && pinned((void**)&sl.mapq, m) && hipEventCreate(&sl.done) == hipSuccess;
    }
    if (!ok) {
        release();
        set_error("push_bam: cannot allocate pinned staging buffers (2 x %lld records)", (long long)chunk_records);
        return BESST_ERR_NOMEM;
    }
    double decode_s = 0.0, wait_s = 0.0;
    int64_t pushed = 0, chunks = 0, bytes = 0;
    const int64_t file_bytes = bam_file_bytes(bam);
    rc = BESST_OK;
    for (int k = 0;; k ^= 1) {
        Slot& sl = slot[k];
        if (sl.busy) {                                       // the copies that last used this slot
            const auto t0 = Clock::now();
            if (hipEventSynchronize(sl.done) != hipSuccess) { set_error("push_bam: a host-to-device copy failed"); rc = BESST_ERR_HIP; break; }
            wait_s += seconds_since(t0);
            sl.busy = false;
        }
        const auto t0 = Clock::now();
        const int64_t got = besst_bam_read_records(bam, chunk_records, sl.tid, sl.mtid, sl.pos, sl.mpos, sl.tlen, sl.flag, sl.mapq,
                                                   sl.qlen, rlen.data(), alen.data());
        decode_s += seconds_since(t0);
        if (got < 0) { rc = (int)-got; break; }              // (the reader has set the error text)
        if (got == 0) break;
        for (int64_t i = 0; i < got && pushed + i < head_records; ++i) {
            head_rlen[pushed + i] = rlen[(size_t)i];
            head_alen[pushed + i] = alen[(size_t)i];
            head_qlen[pushed + i] = sl.qlen[i];
        }
        const int64_t have = c->n_records + pushed;
        if (have + got >= ((int64_t)1 << 32)) { set_error("more than 2^32-1 records in one context"); rc = BESST_ERR_ARG; break; }
        if ((size_t)(have + got) > c->tid.cap &&
            (rc = reserve_records(c, have, column_room(c->n_records, pushed + got, bam_file_position(bam), file_bytes))))
            break;
        const size_t m = (size_t)got;
        hipError_t e = hipSuccess;
        auto up = [&](void* dst, const void* src, size_t nbytes) {
            if (e == hipSuccess) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, c->stream);
            bytes += (int64_t)nbytes;
        };
        up(c->tid.p + have, sl.tid, m * 4); up(c->mtid.p + have, sl.mtid, m * 4); up(c->pos.p + have, sl.pos, m * 4);
        up(c->mpos.p + have, sl.mpos, m * 4); up(c->tlen.p + have, sl.tlen, m * 4); up(c->flag.p + have, sl.flag, m * 2);
        up(c->mapq.p + have, sl.mapq, m); up(c->qlen.p + have, sl.qlen, m * 2);
        if (e == hipSuccess) e = hipEventRecord(sl.done, c->stream);
        if (e != hipSuccess) { set_error("push_bam: %s", hipGetErrorString(e)); rc = BESST_ERR_HIP; break; }
        sl.busy = true;
        pushed += got;
        ++chunks;
    }
    const auto tw = Clock::now();
    const hipError_t es = hipStreamSynchronize(c->stream);
    wait_s += seconds_since(tw);
    release();
    if (rc == BESST_OK && es != hipSuccess) { set_error("push_bam: %s", hipGetErrorString(es)); rc = BESST_ERR_HIP; }
    if (rc) return rc;
    c->n_records += pushed;
    c->built = false;
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->records = pushed;
        stats->chunks = chunks;
        stats->bytes_h2d = bytes;
        stats->seconds = seconds_since(t_start);
        stats->decode_seconds = decode_s;
        stats->copy_wait_seconds = wait_s;
    }
    return BESST_OK;
}

// ---- BAM ingest on the GPU (bgzf_gpu.hip) ----------------------------------------------------------------------------
// BAM file -> resident records with the inflate and the record decode on the GPU: the file's COMPRESSED bytes are read into
// pinned memory by the reader's threads and uploaded chunk by chunk; per chunk one wave per BGZF block inflates, one lane per
// block walks its records, a scan places them and a thread per record fills the columns.  Three slots, each with its own
// staging, scratch and stream: chunk j + 1 is INFLATING and chunk j + 2 read, uploaded and queued behind it while the host
// waits for chunk j's record count (the columns may have to grow before its decode) - the tail of one chunk's waves and the
// head of the next share the chip.  Any block layout: a chunk's blocks are inflated back to back behind a slot that receives the record the chunk before
// left unfinished, and the record starts are guessed per block and verified from block to block (bgzf_gpu.hip).  A block
// the device cannot inflate returns BESST_ERR_UNSUPPORTED with context and reader untouched, and the caller takes
// besst_ctx_push_bam.
namespace {

constexpr int kSlots = 3;            // chunk j's starts being verified, j + 1 inflating, j + 2 on its way to the device
constexpr size_t kTailRoom = kBgzfTailRoom;
enum SlotEvent { kH2dDone = 0, kSlotFree, kSummDone, kTailTaken, kScanDone, kSlotEvents };

// What every device ingest needs whatever the file: four streams (4 ms each to create: 17 of a call's 18 ms of set-up), fifteen
// events and three small buffers.  One set per device stays with the process; a call takes it (a second call on the same
// device at the same time makes its own and destroys it), besst_release_cached_memory() does not touch it (a few KB).
struct IngestHandles {
    hipStream_t work[kSlots] = {}, copy = nullptr;
    hipEvent_t ev[kSlots][kSlotEvents] = {};
    char* heads = nullptr;           // head_rlen | head_alen | head_qlen on the device
    size_t heads_bytes = 0;
    uint32_t* d_flags = nullptr;     // corrupt-record bit, saturated-qlen count | the layout's state: entries did not fit, entries so far
    uint32_t* summ_host = nullptr;   // pinned: kSlots x 12 summary words | [40] .. [43] flag words | [44] entries before the call | [45] entries so far, read where the columns grow | [48..] kSlots tail descriptors
};
struct IngestKit {
    std::mutex mu;
    bool busy = false;
    IngestHandles h;                 // (empty while a call holds them)
};
IngestKit g_ingest_kit[16];

// a work stream at `priority` and the five events of its slot, where they are missing
bool make_slot_handles(hipStream_t* work, hipEvent_t* ev, int priority) {
    if (!*work && hipStreamCreateWithPriority(work, hipStreamNonBlocking, priority) != hipSuccess) return false;
    for (int i = 0; i < kSlotEvents; ++i)
        if (!ev[i] && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
    return true;
}

// What a chunk's walk reports (the 12 summary words of bgzf_gpu.hip, the first ten of them in use).
struct ChunkSummary {
    uint32_t records;
    bool located;                    // every record start verified
    uint32_t block;                  // located: the starts that were repaired; else the first block that is not verified ...
    uint32_t inflate_status;         // ... and its inflate status
    uint32_t tail_len;               // bytes of the record the chunk does not finish,
    uint64_t tail_at;                // and where they begin in the chunk's buffer
    bool straddles;                  // some block begins inside a record (not htslib's layout)
    uint64_t first_at;               // where the chunk's first record begins (~0: nowhere); overhang: bytes of the tail record
    explicit ChunkSummary(const uint32_t* w)
        : records(w[0]), located(w[1] != 0), block(w[2]), inflate_status(w[3]), tail_len(w[4]), tail_at((uint64_t)w[5] | ((uint64_t)w[6] << 32)),
          straddles(w[7] != 0), first_at((uint64_t)w[8] | ((uint64_t)w[9] << 32)) {}
};

struct Chunk { uint32_t n_blocks = 0, first_off = 0; size_t comp = 0, inflated = 0, file_end = 0; };
struct Slot {
    char* pin = nullptr;         // pinned: descriptors, then the chunk's bytes as they lie in the file
    char* dev = nullptr;         // the same on the device
    uint8_t* inflated = nullptr;
    uint32_t* symbols = nullptr; // the inflate kernel's symbol buffer: four bytes per byte of `inflated` (touched: per symbol)
    uint16_t* offs = nullptr;
    uint32_t* words = nullptr;   // status | count | exits | rec_base | guess | tail_at (nbw each), 12 summary words, then set_count | ent_base (nbw each)
    Chunk ck;
};

// One call of the device ingest.  first_skip / slice: the slice form (besst_ctx_push_bam_device_slice; else the part form,
// which takes htslib's layout only and begins every part with its first block's first byte).
struct DeviceIngest {
    // the call
    besst_ctx* const c;
    besst_bam* const bam;
    const int32_t part, parts;
    const int64_t head_records, first_skip;
    const bool slice;
    const Clock::time_point t_start = Clock::now();
    // the plan
    size_t f0 = 0, map_len = 0, whole_file = 0;      // this call's part of the file (map_len: its end), and the file's end
    uint32_t u0 = 0;
    BgzfChunkPlan plan{};
    size_t head_n = 1;
    int32_t n_ref = 0;
    // the three slots, and the handles they share
    Slot sl[kSlots];
    IngestHandles h;
    IngestKit* kit = nullptr;        // the device's cached streams / events / small buffers, if no other call holds them
    BamColumns col{};
    std::thread alloc_helper;
    std::atomic<bool> helper_ok{true};
    // where the call stands
    int rc = BESST_OK;
    size_t fpos = 0;
    double bytes_per_block = 0.0;
    size_t max_blocks = 0;           // (blocks per chunk: fewer for the blocks behind a part's end)
    bool overhang = false;           // the chunk at hand holds the blocks behind the part's end
    int64_t pushed = 0, chunks = 0, comp_total = 0, inflated_total = 0, blocks_total = 0, repaired = 0;
    double setup_s = 0.0, alloc_s = 0.0, stage_s = 0.0, wait_s = 0.0, unpin_s = 0.0;
    double alloc_wait_s = 0.0;       // (what the calling thread spent waiting for the helper)
    // the slice form's answers
    int64_t first_at = -1, carry_out = 0, over_bytes = 0;
    int64_t no_start_left = -1;      // >= 0: a slice no record begins in; so many bytes of the record before lie behind it
    // The layout step (BESST_INGEST_LAYOUT=0: none of it): the decode writes the mate-elsewhere and run planes, and the set
    // plane, the offsets and the entries of the candidate side stream - each only where the context's own watermark stands
    // at its last record, so that what the call writes continues what is valid (else the next build extends it as ever).
    bool lay_planes = false, lay_stream = false;
    int64_t cap_before = 0;          // entries the columns held room for when the call began (a failed call puts that back)
    int64_t cap_limit = INT64_MAX;   // BESST_INGEST_ENTRY_ROOM: the kernels take the columns for no longer than this until they are carved by share
    bool stream_began = false;       // lay_stream when the call began (it is given up where its buffers cannot be allocated)
    int64_t entries_before = 0;      // entries of the records that were resident
    int64_t entry_room = -1;         // BESST_INGEST_ENTRY_ROOM: entries the columns are first carved for (< 0: the default share)
    std::vector<int64_t> seams;      // record index of every chunk's first record

    DeviceIngest(besst_ctx* c_, besst_bam* bam_, int32_t part_, int32_t parts_, int64_t head_records_, int64_t first_skip_, bool slice_)
        : c(c_), bam(bam_), part(part_), parts(parts_), head_records(head_records_), first_skip(first_skip_), slice(slice_) {}

    void hip_fail(hipError_t e) { set_error("push_bam_device: %s", hipGetErrorString(e)); rc = BESST_ERR_HIP; }
    void alloc_fail() {
        set_error("push_bam_device: cannot allocate the staging / scratch buffers (%zu MB pinned, %zu MB of HBM)", (kSlots * plan.slot_bytes) >> 20,
                  (kSlots * (plan.slot_bytes + plan.inflated_cap + 4 * bgzf_inflate_symbol_places(plan.inflated_cap, plan.nbw))) >> 20);
        rc = BESST_ERR_NOMEM;
    }

    // The memory of slot k.  (The only thing the helper thread does: no stream or event handle is written here.)
    bool alloc_slot(int k) {
        Slot& q = sl[k];
        if (q.pin) return true;
        const auto t0 = Clock::now();
        const bool got = (q.pin = static_cast<char*>(g_pinned.acquire(plan.slot_bytes))) != nullptr &&
             hipMalloc((void**)&q.dev, plan.slot_bytes) == hipSuccess && hipMalloc((void**)&q.inflated, plan.inflated_cap) == hipSuccess &&
             hipMalloc((void**)&q.symbols, 4 * bgzf_inflate_symbol_places(plan.inflated_cap, plan.nbw)) == hipSuccess &&
             hipMalloc((void**)&q.offs, plan.nbw * (size_t)kBamBlockRecs * sizeof(uint16_t)) == hipSuccess &&
             hipMalloc((void**)&q.words, (plan.nbw * 8 + 12) * sizeof(uint32_t)) == hipSuccess;
        alloc_s += seconds_since(t0);
        return got;
    }
    bool alloc_join() {
        if (alloc_helper.joinable()) {
            const auto t0 = Clock::now();
            alloc_helper.join();
            alloc_wait_s += seconds_since(t0);
        }
        return helper_ok.load();
    }

    // The device's kit if it is free, and whatever handle is still missing.
    // The three slots' streams and the copy stream must run beside each other.  The runtime spreads a process's streams
    // over a handful of hardware queues PER PRIORITY LEVEL, in creation order, together with every other stream of the
    // process (the context's, the caller's: torch's): two of ours on one queue and chunk j's walk / scan / decode wait
    // behind chunk j + 1's whole inflate - 1.83 instead of 1.40 s for full-size C3 in a process that had made other
    // streams before, 1.40 in one that had not.  So the slots' streams are created at the LOWEST priority, a level nobody
    // else in the process uses (its queues are theirs alone; nothing else runs during an ingest for them to yield to), and
    // the copy stream at the highest - the slots' first, in slot order: the queue placement depends on it.
    // Every slot's stream AND its five events are made here, on the calling thread, before anything is queued: the helper
    // only allocates memory, so no handle the queueing code reads - slot 2's tail_taken while chunk 0 is enqueued - is ever
    // written beside it.
    bool take_handles() {
        int prio_low = 0, prio_high = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
        if (c->device >= 0 && c->device < 16) {
            IngestKit& k = g_ingest_kit[c->device];
            std::lock_guard<std::mutex> g(k.mu);
            if (!k.busy) { k.busy = true; kit = &k; }
        }
        if (kit) {                                               // what an earlier call on this device left
            h = kit->h;
            kit->h = IngestHandles();
            if (h.heads_bytes < head_n * 10) {
                if (h.heads) (void)hipFree(h.heads);
                h.heads = nullptr;
                h.heads_bytes = 0;
            }
        }
        for (int k = 0; k < kSlots; ++k)
            if (!make_slot_handles(&h.work[k], h.ev[k], prio_low)) return false;
        if (!h.heads) {
            if (hipMalloc((void**)&h.heads, head_n * 10) != hipSuccess) return false;
            h.heads_bytes = head_n * 10;
        }
        return (h.d_flags || hipMalloc((void**)&h.d_flags, 4 * sizeof(uint32_t)) == hipSuccess) &&
               (h.summ_host || hipHostMalloc((void**)&h.summ_host, 128 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess) &&
               (h.copy || hipStreamCreateWithPriority(&h.copy, hipStreamNonBlocking, prio_high) == hipSuccess);
    }

    // What the call allocated goes back when it ends: the pinned staging to its pool at once; the device scratch - and, of a
    // call that had no kit, events and streams: 12-15 ms of hipFree / destroy calls, a tenth of a 40 M-record ingest - on a
    // thread of their own (`clean`: the successful end; every stream has been synchronised by then), nobody waits for it.
    void release(bool clean) {
        std::vector<void*> dev_mem, host_mem;
        std::vector<hipEvent_t> events;
        std::vector<hipStream_t> streams;
        for (Slot& q : sl) {
            const auto t0 = Clock::now();
            g_pinned.give_back(q.pin);
            unpin_s += seconds_since(t0);
            for (void* m : {(void*)q.dev, (void*)q.inflated, (void*)q.symbols, (void*)q.offs, (void*)q.words})
                if (m) dev_mem.push_back(m);
            q = Slot();
        }
        if (kit && clean) {                                  // (a call that synchronised cleanly: its handles serve the next one)
            kit->h = h;
        } else {
            // a call that did not end cleanly: a stream or event of it may be in an error state (a failed copy or kernel), and
            // a handle kept for the process would hand that state to every later ingest on this device.  Nothing is cached:
            // the kit's handles are destroyed with the call's own, the next call makes fresh ones.
            for (int k = 0; k < kSlots; ++k) {
                for (hipEvent_t e : h.ev[k])
                    if (e) events.push_back(e);
                if (h.work[k]) streams.push_back(h.work[k]);
            }
            if (h.copy) streams.push_back(h.copy);
            if (h.heads) dev_mem.push_back(h.heads);
            if (h.d_flags) dev_mem.push_back(h.d_flags);
            if (h.summ_host) host_mem.push_back(h.summ_host);
        }
        if (kit) {
            std::lock_guard<std::mutex> g(kit->mu);
            kit->busy = false;
        }
        kit = nullptr;
        h = IngestHandles();
        const int device = c->device;
        auto drop = [device, dev_mem, host_mem, events, streams]() {
            (void)hipSetDevice(device);
            for (hipEvent_t e : events) (void)hipEventDestroy(e);
            for (hipStream_t st : streams) (void)hipStreamDestroy(st);
            for (void* m : dev_mem) (void)hipFree(m);
            for (void* m : host_mem) (void)hipHostFree(m);
        };
        if (clean) g_background.run(drop);
        else drop();
    }

    // Which parts of the layout this call continues, read at every call like the other switches.
    void plan_layout() {
        const char* sw = getenv("BESST_INGEST_LAYOUT");
        const bool on = !(sw && sw[0] == '0' && sw[1] == 0);
        lay_planes = on && c->bits_upto == c->n_records && c->tid_bits_upto == c->n_records;
        lay_stream = lay_planes && c->cs_upto == c->n_records && (c->n_records == 0 || c->cs.n_refs == (int64_t)n_ref);
        stream_began = lay_stream;
        cap_before = c->cs_cap_entries;
        entries_before = lay_stream && c->n_records > 0 ? c->cs.n_entries : 0;
        if (const char* e = getenv("BESST_INGEST_ENTRY_ROOM"); e && e[0]) entry_room = atoll(e) < 0 ? 0 : atoll(e);
    }

    // The planes, the offsets and the entry columns fit the record columns' capacity; `have` records' worth of them is
    // valid and moves along, the rest of the planes is zero.  Called where the record columns may have grown - every slot
    // has been waited for there, so the running entry total can be read.
    // The entry columns' size is known only at the end.  They are carved for what is there plus the room left in the
    // record columns times the share of records that got an entry so far, plus a quarter (layout_entry_cap), and only
    // ever grow.  Before a count has come back the share is kLayoutDefaultShare - every record: that first carving cannot
    // be too small (BESST_INGEST_ENTRY_ROOM replaces it: so many entries).  Behind a growth the rest of the file may hold
    // more entries per record than its head by more than the margin: entries that do not fit raise the state's flag and
    // are not written, and the build makes the stream.
    bool fit_layout(int64_t have) {
        if (!lay_planes) return true;
        const size_t room = c->tid.cap > (size_t)have ? c->tid.cap : (size_t)have;
        const size_t plane_bytes = (room / 8 + 32 + 15) / 16 * 16, keep = (size_t)((have + 7) / 8);
        if ((rc = regrow_zeroed(c, c->mate_bits, keep, plane_bytes)) || (rc = regrow_zeroed(c, c->tid_bits, keep, plane_bytes))) return false;
        if (!lay_stream) return true;
        const bool ok = fit_stream(have, room, keep, plane_bytes);
        point_stream(c);                                         // (on every way out: a buffer may have moved before another failed)
        return ok;
    }

    // the stream's part of fit_layout.  Memory that is not there costs the stream, not the call: the planes go on, cs_upto
    // stays where it was and the build makes the stream, as after entries that did not fit.
    bool fit_stream(int64_t have, size_t room, size_t keep, size_t plane_bytes) {
        auto gave_up = [&](int status) {
            if (status != BESST_ERR_NOMEM) return false;
            (void)hipGetLastError();                             // (the failed allocation's error is not the next launch's)
            lay_stream = false;
            rc = BESST_OK;
            return true;
        };
        if ((rc = regrow_zeroed(c, c->cs_set, keep, plane_bytes))) return gave_up(rc);
        const size_t off_keep = have > 0 ? (size_t)((have + kLayoutTile - 1) / kLayoutTile + 1) : 0;
        if ((rc = regrow_zeroed(c, c->cs_off, off_keep, (room / kLayoutTile + 2 + 3) / 4 * 4))) return gave_up(rc);
        int64_t total = entries_before;
        if (pushed > 0) {
            hipError_t e = hipMemcpyAsync(h.summ_host + 45, h.d_flags + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { hip_fail(e); return false; }
            total = (int64_t)h.summ_host[45];
        }
        int64_t want;
        if (pushed == 0 && entry_room >= 0) {
            want = (total + entry_room + 1 + 63) / 64 * 64;
            cap_limit = want;                                    // (columns that hold more from an earlier call count as this long)
        } else {
            cap_limit = INT64_MAX;
            const double share = pushed > 0 ? (double)(total - entries_before) / (double)pushed : kLayoutDefaultShare;
            want = layout_entry_cap(total, (int64_t)room - have, share);
        }
        if (want > c->cs_cap_entries && (rc = carve_entries(c, want, total))) return gave_up(rc);
        return true;
    }

    // every plane bit at and behind the context's last record is 0 (before the first decode, and again after a call that
    // failed: the planes are ORed into, and the next call must find zeros)
    bool clear_planes() {
        if (!lay_planes) return true;
        uint8_t* const planes[3] = {c->mate_bits.p, c->tid_bits.p, stream_began ? c->cs_set.p : nullptr};
        const size_t caps[3] = {c->mate_bits.cap, c->tid_bits.cap, c->cs_set.cap};
        return launch_plane_clear_from(c->stream, planes, caps, c->n_records) == BESST_OK;
    }

    // The part of the file, its chunks, the handles and slot 0.  false: the call ends here (rc, nothing left allocated).
    bool setup(int64_t chunk_blocks) {
        int64_t at = 0;
        if (!bam_record_position(bam, &at, &u0)) {
            set_error("push_bam_device: the reader is inside a record that straddles two batches");
            rc = BESST_ERR_UNSUPPORTED;
            return false;
        }
        whole_file = (size_t)bam_file_bytes(bam);
        const BgzfPart mine = cut_bgzf_part(bam_file_map(bam), whole_file, (size_t)at, u0, part, parts);
        f0 = mine.begin;
        map_len = mine.end;
        u0 = mine.u0;
        plan = plan_bgzf_chunks(bam_file_map(bam), map_len, f0, (size_t)chunk_blocks);
        head_n = (size_t)(head_records > 0 ? head_records : 1);
        n_ref = besst_bam_n_references(bam);
        plan_layout();
        if (!fit_layout(c->n_records)) return false;             // (rc is set; nothing of the call's is allocated yet)
        // Slot 0 now; slots 1 and 2 - 2 x (~190 MB pinned + ~0.7 GB of HBM): 90 of the 130 ms a first ingest spent allocating -
        // on a helper thread while the first chunk is read, uploaded and queued (joined before the second chunk is staged, and
        // before anything is released).
        const bool ok = take_handles() && alloc_slot(0);
        if (ok && map_len - f0 > plan.comp_cap / 2) {            // (a file of less than a chunk or so never uses them)
            const int device = c->device;
            alloc_helper = std::thread([this, device] {
                if (hipSetDevice(device) != hipSuccess) { helper_ok = false; return; }
                for (int k = 1; k < kSlots; ++k)
                    if (!alloc_slot(k)) { helper_ok = false; return; }
            });
        }
        if (!ok) {
            release(false);
            alloc_fail();
            return false;
        }
        fpos = f0;
        bytes_per_block = plan.first_per_block;
        max_blocks = plan.nb;
        col.head_rlen = reinterpret_cast<int32_t*>(h.heads);
        col.head_alen = reinterpret_cast<int32_t*>(h.heads + head_n * 4);
        col.head_qlen = reinterpret_cast<uint16_t*>(h.heads + head_n * 8);
        hipError_t e = hipMemsetAsync(h.d_flags, 0, 4 * sizeof(uint32_t), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h.heads, 0, head_n * 10, c->stream);
        if (e == hipSuccess && entries_before) {                 // the running entry total goes on from the resident stream's
            h.summ_host[44] = (uint32_t)entries_before;
            e = hipMemcpyAsync(h.d_flags + 3, h.summ_host + 44, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess && !clear_planes()) rc = BESST_ERR_HIP;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the slots' streams start behind these
        if (e != hipSuccess) hip_fail(e);
        setup_s = seconds_since(t_start);
        return true;
    }

    // read chunk j (the next blocks of the file) into slot j % kSlots and start its upload
    bool stage(int64_t j) {
        const int k = (int)(j % kSlots);
        Slot& q = sl[k];
        if (fpos >= map_len) { q.ck = Chunk(); return true; }   // (nothing left: the slot is not touched)
        if ((j > 0 && !alloc_join()) || !alloc_slot(k)) {
            alloc_fail();
            return false;
        }
        if (j >= kSlots) {                                        // the upload that last read this pinned slot
            const auto t0 = Clock::now();
            const hipError_t e = hipEventSynchronize(h.ev[k][kH2dDone]);
            wait_s += seconds_since(t0);
            if (e != hipSuccess) { hip_fail(e); return false; }
        }
        const auto t0 = Clock::now();
        const size_t begin = fpos;
        q.ck = Chunk();
        q.ck.first_off = j == 0 ? u0 : 0u;
        // A window of the file is READ into the pinned slot by the reader's threads (pread: no page faults, unlike a copy
        // off the mapping, where the header walk alone touched every page) and the block headers are walked there; the
        // window is sized from the blocks seen so far, the block it cuts is read again with the next chunk.
        size_t want = map_len - begin < plan.comp_cap ? map_len - begin : plan.comp_cap;
        // the first two chunks are short ones - a fifth and a half of a chunk -, so that the chip has something to inflate a
        // millisecond or two into the call instead of after a whole chunk's read and upload (40 M records, eight calls
        // each way on one box: 0.119 against 0.125 s); the window of the very first read is sized from the file's first
        // blocks (bytes_per_block starts at their average)
        size_t cap_blocks = max_blocks;
        if (!overhang && j < 2) {
            cap_blocks = j == 0 ? plan.nb / 5 : plan.nb / 2;
            if (cap_blocks < 64) cap_blocks = plan.nb < 64 ? plan.nb : 64;
        }
        if (bytes_per_block > 0.0) {
            const size_t guess = (size_t)((double)cap_blocks * bytes_per_block * 1.08) + 65536;
            if (guess < want) want = guess;
        }
        if (!bam_parallel_read(bam, q.pin + plan.desc_bytes, (int64_t)begin, want)) {
            set_error("push_bam_device: reading the file failed at offset %zu", begin);
            rc = BESST_ERR_ARG;
            return false;
        }
        size_t used = 0;
        BgzfBlock* desc = reinterpret_cast<BgzfBlock*>(q.pin);
        desc[0] = BgzfBlock{0u, 0u, (uint32_t)kTailRoom, 0u, 0u, 0u};   // the tail slot: empty until the chunk before says otherwise
        if (!scan_bgzf_chunk(reinterpret_cast<const uint8_t*>(q.pin + plan.desc_bytes), want, &used, cap_blocks, plan.comp_cap, desc + 1,
                             &q.ck.n_blocks, &q.ck.comp, &q.ck.inflated, begin + want < map_len, kTailRoom, true) ||
            (q.ck.n_blocks == 0 && want > 0)) {
            set_error("push_bam_device: not a BGZF block at file offset %zu", begin + used);
            rc = BESST_ERR_UNSUPPORTED;
            return false;
        }
        fpos = begin + q.ck.comp;
        q.ck.file_end = fpos;
        bytes_per_block = (double)q.ck.comp / (double)q.ck.n_blocks;
        stage_s += seconds_since(t0);
        hipError_t e = hipSuccess;
        if (j >= kSlots) e = hipStreamWaitEvent(h.copy, h.ev[k][kSlotFree], 0);    // the kernels that last read this device slot
        if (e == hipSuccess) e = hipMemcpyAsync(q.dev, q.pin, ((size_t)q.ck.n_blocks + 1) * sizeof(BgzfBlock), hipMemcpyHostToDevice, h.copy);
        if (e == hipSuccess) e = hipMemcpyAsync(q.dev + plan.desc_bytes, q.pin + plan.desc_bytes, q.ck.comp + 1024, hipMemcpyHostToDevice, h.copy);
        if (e == hipSuccess) e = hipEventRecord(h.ev[k][kH2dDone], h.copy);
        if (e != hipSuccess) { hip_fail(e); return false; }
        comp_total += (int64_t)q.ck.comp;
        inflated_total += (int64_t)q.ck.inflated;
        blocks_total += q.ck.n_blocks;
        return true;
    }

    // inflate + CRC of the chunk in slot k on the slot's stream (descriptor 0, the tail slot, is empty here: skipped)
    bool enqueue_inflate(int k) {
        Slot& q = sl[k];
        hipError_t e = hipStreamWaitEvent(h.work[k], h.ev[k][kH2dDone], 0);
        // (the chunk two before inflated into this buffer; its tail may still be on its way to the chunk in between)
        if (e == hipSuccess) e = hipStreamWaitEvent(h.work[k], h.ev[k][kTailTaken], 0);
        if (e != hipSuccess) { hip_fail(e); return false; }
        if (launch_bgzf_inflate(h.work[k], reinterpret_cast<const uint8_t*>(q.dev + plan.desc_bytes), reinterpret_cast<const BgzfBlock*>(q.dev),
                                q.ck.n_blocks + 1, q.inflated, q.words, q.symbols)) {
            rc = BESST_ERR_HIP;
            return false;
        }
        return true;
    }

    // where the records of the chunk in slot k begin (entry guesses, walks, verification, scan), its summary on the way to the
    // host.  tail_len bytes at `tail_at` of the buffer of the slot BEFORE are the record the chunk before did not finish: they
    // are copied in front of this chunk's first block and become its block 0.  forced_entry: where the first record begins
    // in block forced_block when there is no tail (the end of the header in the file's first chunk, else 0).
    bool enqueue_walk(int k, uint64_t tail_at, uint32_t tail_len, uint32_t forced_block, uint32_t forced_entry, uint32_t mode) {
        Slot& q = sl[k];
        const int before = (k + kSlots - 1) % kSlots;
        const size_t nbw = plan.nbw;
        uint32_t* w = q.words;
        hipError_t e = hipSuccess;
        if (tail_len) {
            BgzfBlock* patch = reinterpret_cast<BgzfBlock*>(h.summ_host + 48) + k;
            *patch = BgzfBlock{0u, 0u, (uint32_t)(kTailRoom - tail_len), 0u, tail_len, 0u};
            e = hipMemcpyAsync(q.dev, patch, sizeof(BgzfBlock), hipMemcpyHostToDevice, h.work[k]);
            if (e == hipSuccess)
                e = hipMemcpyAsync(q.inflated + kTailRoom - tail_len, sl[before].inflated + tail_at, tail_len, hipMemcpyDeviceToDevice, h.work[k]);
        }
        if (e == hipSuccess) e = hipEventRecord(h.ev[before][kTailTaken], h.work[k]);
        if (e != hipSuccess) { hip_fail(e); return false; }
        if (launch_bam_walk_scan(h.work[k], q.inflated, reinterpret_cast<const BgzfBlock*>(q.dev), q.ck.n_blocks + 1,
                                 (uint64_t)kTailRoom + q.ck.inflated, n_ref, tail_len ? 0xffffffffu : forced_block, forced_entry, mode, w, q.offs,
                                 w + nbw, w + 2 * nbw, w + 3 * nbw, w + 4 * nbw, w + 5 * nbw, w + 6 * nbw)) {
            rc = BESST_ERR_HIP;
            return false;
        }
        e = hipMemcpyAsync(h.summ_host + 12 * k, w + 6 * nbw, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost, h.work[k]);
        if (e == hipSuccess) e = hipEventRecord(h.ev[k][kSummDone], h.work[k]);
        if (e != hipSuccess) { hip_fail(e); return false; }
        return true;
    }

    // Chunk 0 staged, inflating and walked, chunk 1 staged and inflating.  Where the first chunk's first record begins: the
    // end of the header / the first byte of a part of a file in htslib's layout; a slice behind the first one: where the
    // caller says (the bytes in front belong to the last record of the slice before), or a guess that the caller will check
    // against what the slice before reports.
    void start() {
        if (!stage(0) || !sl[0].ck.n_blocks) return;
        uint32_t block = 1u, entry = u0, mode = 0u;
        if (slice && part > 0 && first_skip < 0) {
            block = 0xffffffffu; entry = 0u; mode = kWalkFirstGuessed;
        } else if (slice && part > 0) {
            const BgzfBlock* desc = reinterpret_cast<const BgzfBlock*>(sl[0].pin);
            uint64_t skip = (uint64_t)first_skip;
            block = 0u;
            for (uint32_t i = 1; i <= sl[0].ck.n_blocks; ++i) {
                if (skip < desc[i].dst_len) { block = i; entry = (uint32_t)skip; break; }
                skip -= desc[i].dst_len;
            }
            if (block == 0u && fpos >= map_len) {
                // the WHOLE slice lies in this chunk and no record begins in it (its blocks are the tail of the record before -
                // or hold nothing: the EOF marker of a file with fewer blocks than ranks): an empty slice, what comes in goes on
                no_start_left = (int64_t)skip;
                sl[0].ck = Chunk();
            } else if (block == 0u) {
                set_error("push_bam_device: the slice's first record begins behind its first chunk (%lld bytes in)", (long long)first_skip);
                rc = BESST_ERR_UNSUPPORTED;
            }
        }
        if (rc == BESST_OK && sl[0].ck.n_blocks && enqueue_inflate(0) && enqueue_walk(0, 0, 0u, block, entry, mode) && stage(1) && sl[1].ck.n_blocks)
            enqueue_inflate(1);
    }

    // What chunk j's walk found: an error, or the slice form's answers it adds to.
    bool read_summary(int64_t j, const ChunkSummary& sm) {
        if (!sm.located) {
            if (sm.inflate_status) set_error("push_bam_device: block %u of chunk %lld did not inflate on the device (status %u)", sm.block ? sm.block - 1u : 0u, (long long)j, sm.inflate_status);
            else set_error("push_bam_device: the records of chunk %lld could not be located on the device (block %u: a record start "
                           "that its neighbours do not confirm, or a corrupt length)", (long long)j, sm.block ? sm.block - 1u : 0u);
            rc = BESST_ERR_UNSUPPORTED;
            return false;
        }
        if (parts > 1 && sm.straddles && !slice) {
            set_error("push_bam_device: a record straddles BGZF blocks (chunk %lld): a part of such a file cannot be cut at a block", (long long)j);
            rc = BESST_ERR_UNSUPPORTED;
            return false;
        }
        if (sm.tail_len > (uint32_t)kTailRoom) {
            set_error("push_bam_device: a record of more than %zu MB", kTailRoom >> 20);
            rc = BESST_ERR_UNSUPPORTED;
            return false;
        }
        if (j == 0) {
            first_at = sm.first_at == ~0ull ? -1 : (int64_t)(sm.first_at - (uint64_t)kTailRoom);
            if (slice && first_at < 0) {
                set_error("push_bam_device: no record begins in the first chunk of the slice");
                rc = BESST_ERR_UNSUPPORTED;
                return false;
            }
        }
        if (overhang) {                                      // bytes of the slice's last record that lie in the next slice
            if (sm.tail_len) over_bytes += (int64_t)sl[j % kSlots].ck.inflated;   // (all of this chunk, and the record goes on)
            else carry_out = over_bytes + (int64_t)(uint32_t)sm.first_at;
        }
        return true;
    }

    // Chunk j + 1's records can be located once chunk j's summary is in: it starts with chunk j's unfinished record, if there
    // is one.  A slice whose last record runs on behind its end reads the blocks that follow for it.
    bool walk_next(int64_t j, const ChunkSummary& sm) {
        const int k1 = (int)((j + 1) % kSlots);
        if (sl[k1].ck.n_blocks) return enqueue_walk(k1, sm.tail_at, sm.tail_len, 1u, 0u, 0u);
        if (sm.tail_len && slice && (overhang ? fpos < whole_file : map_len < whole_file)) {
            // the slice's last record runs on behind the slice's end: the blocks that follow are inflated for its bytes (and for
            // nothing else: the records that begin in them are the next slice's) - chunk after chunk until the record ends
            // (a few blocks at first - a record seldom runs over more than one or two -, four times as many while it goes on: the
            // blocks belong to the next slice, and a damaged one among them is that slice's to report)
            max_blocks = overhang ? (max_blocks * 4 < plan.nb ? max_blocks * 4 : plan.nb) : (plan.nb < 64 ? plan.nb : 64);
            overhang = true;
            map_len = whole_file;
            sl[(j + 2) % kSlots].ck = Chunk();
            if (!stage(j + 1)) return false;
            if (!sl[k1].ck.n_blocks) { set_error("push_bam_device: the file ends inside a record"); rc = BESST_ERR_ARG; return false; }
            return enqueue_inflate(k1) && enqueue_walk(k1, sm.tail_at, sm.tail_len, 0xffffffffu, 0u, kWalkOverhang);
        }
        if (sm.tail_len) {
            set_error("push_bam_device: the %s ends inside a record", parts > 1 ? "part of the file" : "file");
            rc = parts > 1 ? BESST_ERR_UNSUPPORTED : BESST_ERR_ARG;
            return false;
        }
        return true;
    }

    // Room for `need` records and more (column_room) before chunk j is decoded; the decode of the chunk before may still be
    // writing the columns that are about to move.
    bool grow_columns(int64_t j, int64_t have, int64_t need) {
        if ((size_t)need <= c->tid.cap) return true;
        const int64_t want = column_room(c->n_records, need - c->n_records, (int64_t)sl[j % kSlots].ck.file_end - (int64_t)f0, (int64_t)(map_len - f0));
        const auto t0 = Clock::now();
        hipError_t e = hipSuccess;
        for (int k = 0; k < kSlots && e == hipSuccess; ++k) e = hipEventSynchronize(h.ev[k][kSlotFree]);   // (behind a slot's last decode)
        wait_s += seconds_since(t0);
        if (e != hipSuccess) { hip_fail(e); return false; }
        return (rc = reserve_records(c, have, want)) == BESST_OK && fit_layout(have);
    }

    // The pipeline: while the host waits for chunk j's summary, chunk j + 1 inflates and chunk j + 2 is read, uploaded and
    // queued behind it; then chunk j + 1 is walked and chunk j decoded.
    void run() {
        if (rc == BESST_OK) start();
        for (int64_t j = 0; rc == BESST_OK && sl[j % kSlots].ck.n_blocks; ++j) {
            const int k = (int)(j % kSlots), k2 = (int)((j + 2) % kSlots);
            Slot& q = sl[k];
            // chunk j + 2: read, uploaded and queued behind chunk j + 1's inflate while chunk j's count is on its way (with two
            // slots the inflate of chunk j + 2 could not be queued before chunk j's verdict had been seen AND the file read:
            // the chip idled between two inflates whenever the two took longer than one inflate)
            if (sl[(j + 1) % kSlots].ck.n_blocks) {
                if (!stage(j + 2)) break;
                if (sl[k2].ck.n_blocks && !enqueue_inflate(k2)) break;
            }
            const auto t0 = Clock::now();
            hipError_t e = hipEventSynchronize(h.ev[k][kSummDone]);
            wait_s += seconds_since(t0);
            if (e != hipSuccess) { hip_fail(e); break; }
            const ChunkSummary sm(h.summ_host + 12 * k);
            if (!read_summary(j, sm) || !walk_next(j, sm)) break;
            const int64_t got = (int64_t)sm.records;
            repaired += (int64_t)sm.block;
            const int64_t have = c->n_records + pushed;
            if (have + got >= ((int64_t)1 << 32)) { set_error("more than 2^32-1 records in one context"); rc = BESST_ERR_ARG; break; }
            if (!grow_columns(j, have, have + got)) break;
            col.tid = c->tid.p; col.mtid = c->mtid.p; col.pos = c->pos.p; col.mpos = c->mpos.p; col.tlen = c->tlen.p;
            col.flag = c->flag.p; col.qlen = c->qlen.p; col.mapq = c->mapq.p;
            BamLayout lay{};
            if (lay_planes) {
                lay.mate = reinterpret_cast<uint32_t*>(c->mate_bits.p);
                lay.runs = reinterpret_cast<uint32_t*>(c->tid_bits.p);
                lay.n_refs = (uint32_t)n_ref;
                seams.push_back(have);
            }
            if (lay_stream) {
                char* ent = reinterpret_cast<char*>(c->cs_entries.p);
                const size_t cap = (size_t)c->cs_cap_entries;
                lay.set = reinterpret_cast<uint32_t*>(c->cs_set.p);
                lay.set_count = q.words + 6 * plan.nbw + 12;
                lay.ent_base = q.words + 7 * plan.nbw + 12;
                lay.state = h.d_flags + 2;
                lay.off = c->cs_off.p;
                lay.e_tid = reinterpret_cast<int32_t*>(ent); lay.e_mtid = reinterpret_cast<int32_t*>(ent + cap * 4);
                lay.e_pos = reinterpret_cast<int32_t*>(ent + cap * 8); lay.e_mpos = reinterpret_cast<int32_t*>(ent + cap * 12);
                lay.e_fq = reinterpret_cast<uint32_t*>(ent + cap * 16); lay.e_mapq = reinterpret_cast<uint8_t*>(ent + cap * 20);
                lay.cap = (uint32_t)((int64_t)cap < cap_limit ? (int64_t)cap : cap_limit);
            }
            const BgzfBlock* desc = reinterpret_cast<const BgzfBlock*>(q.dev);
            if (launch_bam_decode(h.work[k], q.inflated, desc, q.ck.n_blocks + 1, q.offs, q.words + plan.nbw,
                                  q.words + 3 * plan.nbw, col, have, pushed, head_records, h.d_flags, lay_planes ? &lay : nullptr)) { rc = BESST_ERR_HIP; break; }
            if (lay_stream) {
                // the chunk's entries go on where the chunk before stopped: its scan waits for that one's on the device,
                // the host for neither
                if (chunks > 0) e = hipStreamWaitEvent(h.work[k], h.ev[(k + kSlots - 1) % kSlots][kScanDone], 0);
                if (e != hipSuccess) { hip_fail(e); break; }
                if (launch_bam_entry_scan(h.work[k], q.ck.n_blocks + 1, lay)) { rc = BESST_ERR_HIP; break; }
                e = hipEventRecord(h.ev[k][kScanDone], h.work[k]);
                if (e != hipSuccess) { hip_fail(e); break; }
                if (launch_bam_entries(h.work[k], q.inflated, desc, q.ck.n_blocks + 1, q.offs, q.words + plan.nbw, q.words + 3 * plan.nbw, have, lay)) { rc = BESST_ERR_HIP; break; }
            }
            e = hipEventRecord(h.ev[k][kSlotFree], h.work[k]);
            if (e != hipSuccess) { hip_fail(e); break; }
            pushed += got;
            ++chunks;
        }
    }

    // Everything synchronised, the head arrays and the flag words fetched, everything released; on success - and only then -
    // the context and the reader move on.
    int finish(int32_t* head_rlen, int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats, int64_t* boundary) {
        const auto tw = Clock::now();
        hipError_t e0 = hipSuccess;
        for (int k = 0; k < kSlots; ++k) {
            const hipError_t e = hipStreamSynchronize(h.work[k]);
            if (e != hipSuccess) e0 = e;
        }
        const hipError_t ec = hipStreamSynchronize(h.copy);
        if (rc == BESST_OK && (e0 != hipSuccess || ec != hipSuccess)) hip_fail(e0 != hipSuccess ? e0 : ec);
        const int64_t n_new = c->n_records + pushed;
        if (rc == BESST_OK && lay_planes && pushed > 0 &&
            launch_bam_layout_seams(c->stream, seams.data(), seams.size(), c->tid.p, n_new, reinterpret_cast<uint32_t*>(c->tid_bits.p),
                                    lay_stream ? c->cs_off.p : nullptr, h.d_flags + 2))
            rc = BESST_ERR_HIP;
        if (rc == BESST_OK) {
            hipError_t e = hipMemcpyAsync(h.summ_host + 40, h.d_flags, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
            const int64_t hn = pushed < head_records ? pushed : head_records;
            if (e == hipSuccess && hn > 0) {
                e = hipMemcpyAsync(head_rlen, col.head_rlen, (size_t)hn * 4, hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(head_alen, col.head_alen, (size_t)hn * 4, hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(head_qlen, col.head_qlen, (size_t)hn * 2, hipMemcpyDeviceToHost, c->stream);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) hip_fail(e);
        }
        wait_s += seconds_since(tw);
        if (rc == BESST_OK && (h.summ_host[40] & 1u)) {
            set_error("push_bam_device: corrupt record (its name and CIGAR do not fit its length)");
            rc = BESST_ERR_ARG;
        }
        const uint32_t saturated = rc == BESST_OK ? h.summ_host[41] : 0u;
        const bool entries_fit = rc == BESST_OK && h.summ_host[42] == 0u;
        const int64_t n_entries = rc == BESST_OK ? (int64_t)h.summ_host[43] : 0;
        const bool stream_kept = rc == BESST_OK && lay_stream && entries_fit;
        bool again = false;
        if (stream_began && !stream_kept && c->n_records > 0) {
            // the resident stream stays as it was - the call failed, its entries did not fit or its buffers could not be had -,
            // but the first record of the block behind it has written its own entry position over that stream's last offset:
            // put it back
            h.summ_host[44] = (uint32_t)entries_before;
            (void)hipMemcpyAsync(c->cs_off.p + (c->n_records + kLayoutTile - 1) / kLayoutTile, h.summ_host + 44, sizeof(uint32_t),
                                 hipMemcpyHostToDevice, c->stream);
            again = true;
        }
        if (rc != BESST_OK && lay_planes) {                      // nothing moves: what the call wrote into the planes goes
            (void)clear_planes();
            again = true;
        }
        if (again) (void)hipStreamSynchronize(c->stream);
        if (rc != BESST_OK && stream_began && c->cs_cap_entries != cap_before) {   // ... and the entry columns are as long as they were
            if (cap_before > 0) {
                (void)carve_entries(c, cap_before, entries_before);
            } else {
                c->cs_entries.release();
                c->cs_cap_entries = 0;
            }
            point_stream(c);
        }
        // The first carving took an entry per reserved record; a library with few candidates gives most of that back now
        // (a copy of the entries there are; a failure leaves the columns as they are).
        if (stream_kept) {
            const int64_t fit = layout_entry_cap(n_entries, 0, 0.0);
            if (c->cs_cap_entries > 2 * fit) (void)carve_entries(c, fit, n_entries);
        }
        const auto t_rel = Clock::now();
        alloc_join();
        release(rc == BESST_OK);
        if (const char* e = getenv("BESST_INGEST_PROFILE"); e && atoi(e))
            fprintf(stderr, "[push_bam_device] setup %.3f s  alloc %.3f s (%.3f of it waited for)  staging %.3f s  waiting %.3f s  release %.3f s (unpinning %.3f)  total %.3f s\n", setup_s, alloc_s, alloc_wait_s, stage_s,
                    wait_s, seconds_since(t_rel), unpin_s, seconds_since(t_start));
        if (rc) return rc;
        c->n_records = n_new;
        c->built = false;
        if (lay_planes) {                                        // the next build finds nothing to make for these records
            c->bits_upto = c->tid_bits_upto = n_new;
            if (stream_kept) {                                   // (else the build makes the stream, as ever)
                c->cs_upto = n_new;
                c->cs.n_refs = (int64_t)n_ref;
                c->cs.n_records = n_new;
                c->cs.n_entries = n_entries;
                point_stream(c);
            }
        }
        bam_mark_consumed(bam, (int64_t)saturated);
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->records = pushed;
            stats->chunks = chunks;
            stats->bytes_h2d = comp_total;
            stats->seconds = seconds_since(t_start);
            stats->decode_seconds = stage_s;
            stats->copy_wait_seconds = wait_s;
            stats->inflated_bytes = inflated_total;
            stats->blocks = blocks_total;
            stats->on_device = 1;
            stats->starts_repaired = (int32_t)(repaired > 0x7fffffff ? 0x7fffffff : repaired);
        }
        if (boundary) {
            if (chunks == 0 && first_at < 0) {                   // a slice without a block (more ranks than blocks): what comes in goes out
                first_at = first_skip > 0 ? first_skip : 0;
                carry_out = no_start_left >= 0 ? no_start_left : first_at;
            }
            boundary[0] = first_at;
            boundary[1] = carry_out;
        }
        return BESST_OK;
    }
};

int push_bam_device_impl(besst_ctx* c, besst_bam* bam, int32_t part, int32_t parts, int64_t chunk_blocks, int64_t head_records,
                         int32_t* head_rlen, int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats,
                         int64_t first_skip, int64_t* boundary) {
    BESST_REQUIRE(c && bam, "push_bam_device: null context or reader");
    BESST_REQUIRE(parts >= 1 && part >= 0 && part < parts, "push_bam_device: part must be in [0, parts)");
    BESST_REQUIRE(head_records >= 0 && (head_records == 0 || (head_rlen && head_alen && head_qlen)),
                  "push_bam_device: head buffers missing");
    if (chunk_blocks <= 0) chunk_blocks = 5120;              // (one full chip of the inflate kernel's waves: 1024 SIMDs x 5; twice that reads 10 % slower)
    if (chunk_blocks < 64) chunk_blocks = 64;
    if (chunk_blocks > 65536) chunk_blocks = 65536;
    int rc = use_device(c);
    if (rc) return rc;
    DeviceIngest ingest(c, bam, part, parts, head_records, first_skip, boundary != nullptr);
    if (!ingest.setup(chunk_blocks)) return ingest.rc;
    ingest.run();
    return ingest.finish(head_rlen, head_alen, head_qlen, stats, boundary);
}

}  // namespace

extern "C" {

int besst_ctx_push_bam_device(besst_ctx* c, besst_bam* bam, int64_t chunk_blocks, int64_t head_records, int32_t* head_rlen,
                              int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats) {
    return besst_ctx_push_bam_device_part(c, bam, 0, 1, chunk_blocks, head_records, head_rlen, head_alen, head_qlen, stats);
}

// The same for ONE PART of the file's records (multi-GPU ingest: rank r of W takes part r of W and holds the r-th slice of
// the stream, which is what phase 1 of the sharded build works on): the file is cut at the BGZF block boundaries nearest
// to part / parts of its bytes - in htslib's layout every block begins with a record, so every boundary is a valid place
// to start, and every rank finds the same boundaries on its own.
int besst_ctx_push_bam_device_part(besst_ctx* c, besst_bam* bam, int32_t part, int32_t parts, int64_t chunk_blocks, int64_t head_records,
                                   int32_t* head_rlen, int32_t* head_alen, uint16_t* head_qlen, besst_ingest_stats* stats) {
    return push_bam_device_impl(c, bam, part, parts, chunk_blocks, head_records, head_rlen, head_alen, head_qlen, stats, -1, nullptr);
}

// Slice `part` of `parts` of a file in ANY block layout (multi-GPU ingest of files whose records straddle BGZF blocks): the
// slices are cut at block boundaries as above, and a record belongs to the slice it BEGINS in.  Where a slice's first record
// begins is the one thing a rank cannot know alone: first_skip < 0 lets it guess (the heuristics of the block-to-block
// verification; everything behind the guess is verified as usual), and boundary[0] reports the offset used - in inflated
// bytes from the slice's first block -, boundary[1] how many bytes of the slice's last record lie in the next slice.  The
// callers exchange these two numbers: slice r is right iff boundary[0] of slice r equals boundary[1] of slice r - 1 (slice 0
// begins behind the header and is always right); a slice whose guess was wrong is read again with first_skip = that
// number (besst_amd.distributed.ingest_slice does this).  The bytes of a slice's last record that lie behind its end are
// read from the blocks that follow (at most 4 MiB).
int besst_ctx_push_bam_device_slice(besst_ctx* c, besst_bam* bam, int32_t part, int32_t parts, int64_t chunk_blocks, int64_t first_skip,
                                    int64_t* boundary, int64_t head_records, int32_t* head_rlen, int32_t* head_alen,
                                    uint16_t* head_qlen, besst_ingest_stats* stats) {
    BESST_REQUIRE(boundary, "push_bam_device_slice: boundary is null");
    return push_bam_device_impl(c, bam, part, parts, chunk_blocks, head_records, head_rlen, head_alen, head_qlen, stats, first_skip,
                                boundary);
}

int besst_bgzf_inflate_device(int device, const void* bgzf, size_t n_bytes, void* out, size_t out_cap, size_t* out_len) {
    BESST_REQUIRE(bgzf && out_len && (out || out_cap == 0), "bgzf_inflate_device: null pointer");
    BESST_HIP_TRY(hipSetDevice(device));
    const uint8_t* map = static_cast<const uint8_t*>(bgzf);
    size_t nb = 4096;                                        // (BESST_INFLATE_HOOK_BLOCKS: blocks per launch, for timing runs)
    if (const char* e = getenv("BESST_INFLATE_HOOK_BLOCKS"); e && atoi(e) > 0) nb = (size_t)atoi(e);
    const size_t comp_cap = nb * 65536;
    std::vector<BgzfBlock> desc(nb);
    std::vector<uint32_t> status(nb);
    std::vector<uint8_t> host;
    char* d_comp = nullptr;
    uint8_t* d_inf = nullptr;
    BgzfBlock* d_desc = nullptr;
    uint32_t* d_status = nullptr;
    uint32_t* d_sym = nullptr;
    auto release = [&]() {
        if (d_comp) (void)hipFree(d_comp);
        if (d_inf) (void)hipFree(d_inf);
        if (d_sym) (void)hipFree(d_sym);
        if (d_desc) (void)hipFree(d_desc);
        if (d_status) (void)hipFree(d_status);
    };
    size_t fpos = 0, written = 0, block0 = 0;
    int rc = BESST_OK;
    while (fpos < n_bytes && rc == BESST_OK) {
        const size_t begin = fpos;
        uint32_t n = 0;
        size_t comp = 0, inflated = 0;
        if (!scan_bgzf_chunk(map, n_bytes, &fpos, nb, comp_cap, desc.data(), &n, &comp, &inflated)) {
            set_error("bgzf_inflate_device: not a BGZF block at offset %zu", fpos);
            rc = BESST_ERR_ARG;
            break;
        }
        if (n == 0) break;
        release();
        d_comp = nullptr; d_inf = nullptr; d_desc = nullptr; d_status = nullptr; d_sym = nullptr;
        hipError_t e = hipMalloc((void**)&d_comp, comp + 4096);
        if (e == hipSuccess) e = hipMalloc((void**)&d_inf, inflated + 4096);
        if (e == hipSuccess) e = hipMalloc((void**)&d_sym, 4 * bgzf_inflate_symbol_places(inflated + 4096, n));
        if (e == hipSuccess) e = hipMalloc((void**)&d_desc, (size_t)n * sizeof(BgzfBlock));
        if (e == hipSuccess) e = hipMalloc((void**)&d_status, (size_t)n * 4);
        if (e == hipSuccess) e = hipMemset(d_comp + comp, 0, 4096);
        if (e == hipSuccess) e = hipMemcpy(d_comp, map + begin, comp, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_desc, desc.data(), (size_t)n * sizeof(BgzfBlock), hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("bgzf_inflate_device: %s", hipGetErrorString(e)); rc = BESST_ERR_HIP; break; }
        if ((rc = launch_bgzf_inflate(nullptr, reinterpret_cast<const uint8_t*>(d_comp), d_desc, n, d_inf, d_status, d_sym))) break;
        host.resize(inflated);
        e = hipMemcpy(status.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && inflated) e = hipMemcpy(host.data(), d_inf, inflated, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_error("bgzf_inflate_device: %s", hipGetErrorString(e)); rc = BESST_ERR_HIP; break; }
        for (uint32_t b = 0; b < n; ++b) {
            if (status[b]) {
                set_error("bgzf_inflate_device: block %zu did not inflate (status %u)", block0 + b, status[b]);
                rc = BESST_ERR_UNSUPPORTED;
                break;
            }
            if (written + desc[b].dst_len > out_cap) { set_error("bgzf_inflate_device: output buffer too small"); rc = BESST_ERR_ARG; break; }
            memcpy(static_cast<uint8_t*>(out) + written, host.data() + (((size_t)desc[b].dst_off_hi << 32) | desc[b].dst_off_lo), desc[b].dst_len);
            written += desc[b].dst_len;
        }
        block0 += n;
    }
    release();
    if (rc) return rc;
    *out_len = written;
    return BESST_OK;
}

int besst_bgzf_walk(const void* bgzf, size_t n_bytes, int64_t max_blocks, int64_t* n_blocks, int64_t* inflated_bytes, size_t* end) {
    BESST_REQUIRE((bgzf || n_bytes == 0) && n_blocks && inflated_bytes && end, "bgzf_walk: null pointer");
    const BgzfWalk w = walk_bgzf(static_cast<const uint8_t*>(bgzf), n_bytes, max_blocks < 0 ? ~(uint64_t)0 : (uint64_t)max_blocks);
    *n_blocks = (int64_t)w.n_blocks;
    *inflated_bytes = (int64_t)w.inflated_bytes;
    *end = w.end;
    return BESST_OK;
}

static_assert(sizeof(besst_bgzf_block) == sizeof(BgzfBlock) && offsetof(besst_bgzf_block, src_len) == offsetof(BgzfBlock, src_len) &&
                  offsetof(besst_bgzf_block, dst_off_lo) == offsetof(BgzfBlock, dst_off_lo) &&
                  offsetof(besst_bgzf_block, dst_off_hi) == offsetof(BgzfBlock, dst_off_hi) &&
                  offsetof(besst_bgzf_block, dst_len) == offsetof(BgzfBlock, dst_len) && offsetof(besst_bgzf_block, crc) == offsetof(BgzfBlock, crc),
              "besst_bgzf_block is BgzfBlock");

int besst_bgzf_scan_chunk(const void* window, size_t n_bytes, size_t from, int32_t more_follows, int64_t max_blocks, uint64_t dst0,
                          besst_bgzf_block* blocks, int64_t* n_blocks, size_t* comp_bytes, int64_t* inflated_bytes) {
    BESST_REQUIRE((window || n_bytes == 0) && n_blocks && comp_bytes && inflated_bytes && (blocks || max_blocks == 0), "bgzf_scan_chunk: null pointer");
    BESST_REQUIRE(from <= n_bytes && n_bytes <= 0xFFFFFFFFull && max_blocks >= 0 && max_blocks <= 0x7FFFFFFF, "bgzf_scan_chunk: sizes out of range");
    BgzfBlock* out = reinterpret_cast<BgzfBlock*>(blocks);
    size_t at = from, comp = 0, inflated = 0;
    uint32_t n = 0;
    if (!scan_bgzf_chunk(static_cast<const uint8_t*>(window), n_bytes, &at, (size_t)max_blocks, ~(size_t)0, out, &n, &comp, &inflated,
                         more_follows != 0, (size_t)dst0, true)) {
        set_error("bgzf_scan_chunk: no whole BGZF block where one should begin");
        return BESST_ERR_ARG;
    }
    for (uint32_t b = 0; b < n; ++b) out[b].src_off += (uint32_t)from;   // (from the window's first byte: the payloads' words stay aligned)
    *n_blocks = (int64_t)n;
    *comp_bytes = comp;
    *inflated_bytes = (int64_t)inflated;
    return BESST_OK;
}

// workspace of a launch: the blocks' status words, then the second form's symbols
static size_t inflate_status_bytes(int64_t n_blocks) { return align_up((size_t)n_blocks * 4, 256); }

size_t besst_dev_bgzf_inflate_workspace_bytes(int64_t n_blocks, int64_t inflated_bytes) {
    if (n_blocks < 0 || n_blocks > ((int64_t)1 << 24) || inflated_bytes < 0 || inflated_bytes > n_blocks * 65536) return 0;
    return inflate_status_bytes(n_blocks) + 4 * bgzf_inflate_symbol_places((size_t)inflated_bytes, (size_t)n_blocks);
}

int besst_dev_bgzf_inflate(void* stream, const void* comp, const besst_bgzf_block* blocks, int64_t n_blocks, int64_t block_base,
                           int64_t inflated_bytes, void* dst, void* workspace, size_t workspace_bytes, uint64_t* first_bad) {
    BESST_REQUIRE(comp && blocks && dst && workspace && first_bad, "dev_bgzf_inflate: null pointer");
    BESST_REQUIRE(block_base >= 0 && block_base < ((int64_t)1 << 55), "dev_bgzf_inflate: block_base out of range");
    const size_t need = besst_dev_bgzf_inflate_workspace_bytes(n_blocks, inflated_bytes);
    BESST_REQUIRE(need != 0, "dev_bgzf_inflate: n_blocks or inflated_bytes out of range");
    BESST_REQUIRE(workspace_bytes >= need, "dev_bgzf_inflate: workspace too small");
    BESST_REQUIRE(((uintptr_t)comp & 3u) == 0 && ((uintptr_t)workspace & 15u) == 0, "dev_bgzf_inflate: comp or workspace misaligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* status = static_cast<uint32_t*>(workspace);
    uint32_t* symbols = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + inflate_status_bytes(n_blocks));
    if (int rc = launch_bgzf_inflate(s, static_cast<const uint8_t*>(comp), reinterpret_cast<const BgzfBlock*>(blocks), (uint32_t)n_blocks,
                                     static_cast<uint8_t*>(dst), status, symbols))
        return rc;
    return launch_bgzf_first_bad(s, status, (uint32_t)n_blocks, (uint64_t)block_base, first_bad);
}

}  // extern "C"
