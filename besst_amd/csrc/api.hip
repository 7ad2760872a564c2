// C ABI of libbesst_amd.so: argument checking, the HBM-owning context, and the host-side float
// finishing that must replay the reference's operation order.  See include/besst_amd.h.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "context.h"

namespace besst {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

struct ProfRec {
    int slot;
    hipEvent_t a, b;
};
static uint32_t g_prof_mask = 0;
static uint32_t g_prof_every = 1;                  // record every n-th launch of an enabled slot
static uint32_t g_prof_seen[kProfSlots] = {};
static std::vector<ProfRec> g_prof;

ProfScope::ProfScope(hipStream_t stream, int slot) : s(stream), idx(-1) {
    if (!((g_prof_mask >> slot) & 1u)) return;
    if ((g_prof_seen[slot]++ % g_prof_every) != 0) return;
    ProfRec r;
    r.slot = slot;
    if (hipEventCreate(&r.a) != hipSuccess) return;
    if (hipEventCreate(&r.b) != hipSuccess) { (void)hipEventDestroy(r.a); return; }
    (void)hipEventRecord(r.a, s);
    g_prof.push_back(r);
    idx = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(g_prof[(size_t)idx].b, s);
}

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int bits_for(uint64_t v) {
    int b = 1;
    while ((v >> b) != 0) ++b;
    return b;
}

}  // namespace

}  // namespace besst

using namespace besst;

namespace {

template <typename T>
int grow_copy(besst_ctx* c, DevBuf<T>& buf, int64_t have, const T* src, int64_t n) {
    if ((size_t)(have + n) > buf.cap) {
        DevBuf<T> bigger;
        int rc = bigger.ensure((size_t)(have + n) * 3 / 2 + 1024);
        if (rc) return rc;
        if (have) BESST_HIP_TRY(hipMemcpyAsync(bigger.p, buf.p, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
        buf.release();
        buf = bigger;
    }
    BESST_HIP_TRY(hipMemcpyAsync(buf.p + have, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return BESST_OK;
}

}  // namespace

extern "C" {

int besst_abi_version(void) { return BESST_ABI_VERSION; }

const char* besst_last_error(void) { return g_error; }

void besst_prof_enable(uint32_t slot_mask) {
    g_prof_mask = slot_mask;
    for (int i = 0; i < kProfSlots; ++i) g_prof_seen[i] = 0;
}

void besst_prof_sample_every(uint32_t n) { g_prof_every = n ? n : 1; }

int besst_prof_slots(void) { return kProfSlots; }

const char* besst_prof_slot_name(int slot) {
    static const char* names[kProfSlots] = {
        "stream_kernel", "fused_wave_kernel", "ordered_kernel", "stitch_spans_kernel+stitch_kernel",
        "presort_fixup_kernel", "compact_kernel",
        "radix_hist_kernel", "radix_rowscan_kernel", "radix_scatter_kernel", "bucket_sort_kernel", "bucket_reduce_kernel",
        "row_heads_kernel", "row_scan_kernel", "row_reduce_kernel",
        "os_hist_kernel", "os_offsets_kernel", "os_seg_tiles_kernel+os_scatter_kernel",
        "os_bucket_start_kernel+os_bucket_wave_kernel+os_bucket_wave_lds_kernel+os_bucket_sort_kernel", "os_bucket_rows_kernel",
        "os_reduce_kernel", "os_fixup_kernel",
        "metrics_kernels", "score_kernels", "rg_group_kernel", "rg_compact_kernel",
        "rg_tile_sums_kernel+rg_dst_kernel(+rg_rows_kernel)", "rg_copy_kernel", "msd_partition_kernel",
        "rl_list_kernel", "rl_place_kernel", "rl_rows_kernel"};
    return (slot >= 0 && slot < kProfSlots) ? names[slot] : "";
}

int besst_prof_collect(int n_slots, double* ms, int64_t* launches) {
    BESST_REQUIRE(ms && launches && n_slots >= kProfSlots, "prof_collect: need kProfSlots entries");
    for (int i = 0; i < n_slots; ++i) { ms[i] = 0.0; launches[i] = 0; }
    int rc = BESST_OK;
    for (ProfRec& r : g_prof) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            ms[r.slot] += (double)t;
            launches[r.slot] += 1;
        } else {
            rc = BESST_ERR_HIP;
        }
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof.clear();
    if (rc) set_error("prof_collect: an event could not be read");
    return rc;
}

int besst_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return -BESST_ERR_HIP;
    }
    return n;
}

besst_ctx* besst_ctx_create(int device) {
    int n = besst_device_count();
    if (n <= 0) {
        if (n == 0) set_error("no HIP device visible");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (have %d)", device, n);
        return nullptr;
    }
    besst_ctx* c = new besst_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) {
        set_error("could not create a stream on device %d", device);
        delete c;
        return nullptr;
    }
    if (c->small.ensure(sizeof(SmallBlock)) != BESST_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

void besst_ctx_destroy(besst_ctx* c) {
    if (!c) return;
    ingest_join_background();
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->table.release(); c->aligned.release();
    c->tid.release(); c->mtid.release(); c->pos.release(); c->mpos.release(); c->tlen.release();
    c->flag.release(); c->qlen.release(); c->mapq.release(); c->mate_bits.release(); c->tid_bits.release();
    c->cs_set.release(); c->cs_off.release(); c->cs_entries.release();
    c->keys.release(); c->payload.release(); c->row_key.release();
    c->row_mask.release(); c->row_n.release(); c->row_first.release(); c->row_offset.release();
    c->row_sum.release(); c->row_sum_sq.release(); c->obs_lo.release(); c->obs_hi.release();
    c->ws.release(); c->small.release(); c->top_mask.release(); c->sample_a.release();
    c->sample_b.release(); c->aux.release(); c->ln_tables.release();
    c->sam_slots.release(); c->sam_rows.release(); c->sam_pool.release(); c->sam_off.release(); c->sam_ws.release();
    c->sam_head.release();
    if (c->side_stream) {
        (void)hipStreamSynchronize(c->side_stream);
        (void)hipStreamDestroy(c->side_stream);
    }
    c->obs_sum.release();
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int besst_dev_pack_contigs(void* stream, int64_t n, const int32_t* scaf_id, const int32_t* scaf_len,
                           const int32_t* ctg_pos, const int32_t* ctg_len, const uint8_t* direction,
                           const uint8_t* cls, void* d_table) {
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "pack_contigs: n_contigs out of range");
    BESST_REQUIRE(n == 0 || (scaf_id && scaf_len && ctg_pos && ctg_len && direction && cls && d_table),
                  "pack_contigs: null pointer");
    std::vector<ContigRow> rows((size_t)n);
    // the class bytes follow the rows, and behind them one byte that says "every contig of the header is in the table"
    // (true for a first library: the record loop then never has to look a class up to know that a record counts)
    std::vector<uint8_t> cls_x((size_t)n + 1);
    uint8_t all_present = 1;
    for (int64_t i = 0; i < n; ++i) {
        BESST_REQUIRE(cls[i] <= BESST_CLS_SMALL, "pack_contigs: class must be 0, 1 or 2");
        cls_x[(size_t)i] = cls[i];
        if (cls[i] == BESST_CLS_ABSENT) all_present = 0;
        if (cls[i] != BESST_CLS_ABSENT)
            BESST_REQUIRE(scaf_id[i] >= 1 && (uint32_t)scaf_id[i] <= kScafIdMask,
                          "pack_contigs: scaffold id must be in [1, 2^28)");
        rows[(size_t)i].w0 = ((uint32_t)scaf_id[i] & kScafIdMask) | ((direction[i] ? 1u : 0u) << 28) |
                             ((uint32_t)cls[i] << 29);
        rows[(size_t)i].scaf_len = scaf_len[i];
        rows[(size_t)i].ctg_pos = ctg_pos[i];
        rows[(size_t)i].ctg_len = ctg_len[i];
    }
    if (n) {
        BESST_HIP_TRY(hipMemcpyAsync(d_table, rows.data(), (size_t)n * sizeof(ContigRow), hipMemcpyHostToDevice,
                                     static_cast<hipStream_t>(stream)));
        // class bytes follow the rows (the streaming kernel needs only the class of a contig)
        cls_x[(size_t)n] = all_present;
        BESST_HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_table) + (size_t)n * sizeof(ContigRow), cls_x.data(), (size_t)n + 1,
                                     hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
        BESST_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // rows is a local
    }
    return BESST_OK;
}

int besst_ctx_set_contigs(besst_ctx* c, int64_t n, const int32_t* scaf_id, const int32_t* scaf_len,
                          const int32_t* ctg_pos, const int32_t* ctg_len, const uint8_t* direction,
                          const uint8_t* cls) {
    BESST_REQUIRE(c, "null context");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = c->table.ensure((size_t)n + (size_t)n / 16 + 2))) return rc;
    if ((rc = c->aligned.ensure((size_t)n + 1))) return rc;
    if ((rc = besst_dev_pack_contigs(c->stream, n, scaf_id, scaf_len, ctg_pos, ctg_len, direction, cls, c->table.p)))
        return rc;
    uint32_t max_id = 1, min_id = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i)
        if (cls[i] != BESST_CLS_ABSENT) {
            if ((uint32_t)scaf_id[i] > max_id) max_id = (uint32_t)scaf_id[i];
            if ((uint32_t)scaf_id[i] < min_id) min_id = (uint32_t)scaf_id[i];
        }
    if (min_id > max_id) min_id = max_id;
    c->node_bits = bits_for((uint64_t)max_id * 2 + 1);
    // every key is >= the one of (lowest node, lowest node): later libraries' scaffold ids start far above 1
    c->key_base = (((uint64_t)min_id * 2) << c->node_bits) << 1;
    c->key_bits = bits_for((((((uint64_t)max_id * 2 + 1) << c->node_bits) | ((uint64_t)max_id * 2 + 1)) << 1 | 1ull) - c->key_base);
    c->n_contigs = n;
    c->built = false;
    return BESST_OK;
}

int besst_ctx_set_library(besst_ctx* c, const besst_lib_params* p) {
    BESST_REQUIRE(c && p, "null pointer");
    BESST_REQUIRE(p->orientation == 0 || p->orientation == 1, "orientation must be 0 (fr) or 1 (rf)");
    BESST_REQUIRE(p->ins_size_threshold < 1073741824.0, "ins_size_threshold must be below 2^30");
    BESST_REQUIRE(p->read_len == p->read_len && p->ins_size_threshold == p->ins_size_threshold, "NaN parameter");
    c->lib = *p;
    c->have_lib = true;
    c->built = false;
    return BESST_OK;
}

int besst_ctx_clear_records(besst_ctx* c) {
    BESST_REQUIRE(c, "null context");
    c->n_records = 0;
    c->bits_upto = 0;
    c->tid_bits_upto = 0;
    c->cs_upto = 0;
    c->built = false;
    return BESST_OK;
}

int besst_ctx_push_records(besst_ctx* c, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                           const int32_t* mpos, const int32_t* tlen, const uint16_t* flag, const uint8_t* mapq,
                           const uint16_t* qlen) {
    BESST_REQUIRE(c, "null context");
    BESST_REQUIRE(n >= 0, "negative record count");
    if (n == 0) return BESST_OK;
    BESST_REQUIRE(tid && mtid && pos && mpos && tlen && flag && mapq && qlen, "null column");
    BESST_REQUIRE(c->n_records + n < ((int64_t)1 << 32), "more than 2^32-1 records in one context");
    int rc = use_device(c);
    if (rc) return rc;
    const int64_t have = c->n_records;
    if ((rc = grow_copy(c, c->tid, have, tid, n))) return rc;
    if ((rc = grow_copy(c, c->mtid, have, mtid, n))) return rc;
    if ((rc = grow_copy(c, c->pos, have, pos, n))) return rc;
    if ((rc = grow_copy(c, c->mpos, have, mpos, n))) return rc;
    if ((rc = grow_copy(c, c->tlen, have, tlen, n))) return rc;
    if ((rc = grow_copy(c, c->flag, have, flag, n))) return rc;
    if ((rc = grow_copy(c, c->mapq, have, mapq, n))) return rc;
    if ((rc = grow_copy(c, c->qlen, have, qlen, n))) return rc;
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));   // caller may reuse its host buffers
    c->n_records += n;
    c->built = false;
    return BESST_OK;
}

int besst_ctx_record_count(besst_ctx* c, int64_t* n) {
    BESST_REQUIRE(c && n, "null pointer");
    *n = c->n_records;
    return BESST_OK;
}

int besst_ctx_record_pointers(besst_ctx* c, int64_t* n, uint64_t* ptrs) {
    BESST_REQUIRE(c && n && ptrs, "null pointer");
    *n = c->n_records;
    const void* p[8] = {c->tid.p, c->mtid.p, c->pos.p, c->mpos.p, c->tlen.p, c->flag.p, c->mapq.p, c->qlen.p};
    for (int k = 0; k < 8; ++k) ptrs[k] = (uint64_t)(uintptr_t)p[k];
    return BESST_OK;
}

int besst_ctx_fetch_records(besst_ctx* c, int64_t first, int64_t n, int32_t* tid, int32_t* mtid, int32_t* pos, int32_t* mpos,
                            int32_t* tlen, uint16_t* flag, uint8_t* mapq, uint16_t* qlen) {
    BESST_REQUIRE(c, "null context");
    BESST_REQUIRE(first >= 0 && n >= 0 && first + n <= c->n_records, "fetch_records: range outside the resident records");
    if (n == 0) return BESST_OK;
    int rc = use_device(c);
    if (rc) return rc;
    auto down = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t m = (size_t)n;
    BESST_HIP_TRY(down(tid, c->tid.p + first, m * 4));
    BESST_HIP_TRY(down(mtid, c->mtid.p + first, m * 4));
    BESST_HIP_TRY(down(pos, c->pos.p + first, m * 4));
    BESST_HIP_TRY(down(mpos, c->mpos.p + first, m * 4));
    BESST_HIP_TRY(down(tlen, c->tlen.p + first, m * 4));
    BESST_HIP_TRY(down(flag, c->flag.p + first, m * 2));
    BESST_HIP_TRY(down(mapq, c->mapq.p + first, m));
    BESST_HIP_TRY(down(qlen, c->qlen.p + first, m * 2));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int besst_ctx_layout_state(besst_ctx* c, int64_t* out) {
    BESST_REQUIRE(c && out, "layout_state: null pointer");
    const bool stream = c->cs_upto > 0;
    out[0] = c->n_records;
    out[1] = c->bits_upto;
    out[2] = c->tid_bits_upto;
    out[3] = c->cs_upto;
    out[4] = stream ? c->cs.n_entries : 0;
    out[5] = stream ? c->cs.n_refs : 0;
    out[6] = c->cs_cap_entries;
    out[7] = c->maker_launches;
    return BESST_OK;
}

int besst_ctx_fetch_layout(besst_ctx* c, uint8_t* mate_bits, uint8_t* tid_bits, uint8_t* set_bits, uint32_t* offsets, int32_t* tid,
                           int32_t* mtid, int32_t* pos, int32_t* mpos, uint32_t* flag_qlen, uint8_t* mapq) {
    BESST_REQUIRE(c, "fetch_layout: null context");
    int rc = use_device(c);
    if (rc) return rc;
    auto down = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    BESST_HIP_TRY(down(mate_bits, c->mate_bits.p, (size_t)((c->bits_upto + 7) / 8)));
    BESST_HIP_TRY(down(tid_bits, c->tid_bits.p, (size_t)((c->tid_bits_upto + 7) / 8)));
    if (c->cs_upto > 0) {
        const size_t m = (size_t)c->cs.n_entries, cap = (size_t)c->cs_cap_entries;
        const uint8_t* e = c->cs_entries.p;
        BESST_HIP_TRY(down(set_bits, c->cs_set.p, (size_t)((c->cs_upto + 7) / 8)));
        BESST_HIP_TRY(down(offsets, c->cs_off.p, (size_t)((c->cs_upto + kClsTile - 1) / kClsTile + 1) * sizeof(uint32_t)));
        BESST_HIP_TRY(down(tid, e, m * 4));
        BESST_HIP_TRY(down(mtid, e + cap * 4, m * 4));
        BESST_HIP_TRY(down(pos, e + cap * 8, m * 4));
        BESST_HIP_TRY(down(mpos, e + cap * 12, m * 4));
        BESST_HIP_TRY(down(flag_qlen, e + cap * 16, m * 4));
        BESST_HIP_TRY(down(mapq, e + cap * 20, m));
    }
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    // the valid prefix only: the bits behind a watermark in the byte that holds it are later records' (or nobody's)
    auto mask_tail = [](uint8_t* plane, int64_t upto) {
        if (plane && (upto & 7)) plane[upto >> 3] &= (uint8_t)((1u << (upto & 7)) - 1u);
    };
    mask_tail(mate_bits, c->bits_upto);
    mask_tail(tid_bits, c->tid_bits_upto);
    if (c->cs_upto > 0) mask_tail(set_bits, c->cs_upto);
    return BESST_OK;
}

size_t besst_dev_classify_workspace_bytes(int64_t n_records) { return classify_workspace_bytes(n_records); }
namespace {
__global__ __launch_bounds__(256) void copy_words_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t n16,
                                                         const uint8_t* __restrict__ src_tail, uint8_t* __restrict__ dst_tail, uint32_t n_tail) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) dst[i] = src[i];
    if (i < n_tail) dst_tail[i] = src_tail[i];
}
}  // namespace

// The state block of a pass (coverage numerators, counters, carry: ~8 bytes per contig) restored from its template at the
// head of every step: one launch of one kernel, a thread per 16 bytes (the runtime's buffer copy took 5.6 us for C2's 80 KB -
// 6 % of that config's whole step).
int besst_dev_restore_state(void* stream, void* dst, const void* src, int64_t bytes) {
    BESST_REQUIRE(bytes >= 0 && (bytes == 0 || (dst && src)), "dev_restore_state: null pointer or negative size");
    BESST_REQUIRE(((uintptr_t)dst & 15u) == 0 && ((uintptr_t)src & 15u) == 0, "dev_restore_state: buffers must be 16-byte aligned");
    if (bytes == 0) return BESST_OK;
    const uint32_t n16 = (uint32_t)(bytes / 16), n_tail = (uint32_t)(bytes % 16);
    const uint32_t blocks = (n16 + 255u) / 256u;
    hipLaunchKernelGGL(copy_words_kernel, dim3(blocks ? blocks : 1u), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4*>(src), static_cast<uint4*>(dst), n16,
                       static_cast<const uint8_t*>(src) + (size_t)n16 * 16, static_cast<uint8_t*>(dst) + (size_t)n16 * 16, n_tail);
    BESST_HIP_TRY(hipGetLastError());
    return BESST_OK;
}

size_t besst_dev_contig_table_bytes(int64_t n_contigs) { return (size_t)(n_contigs > 0 ? n_contigs : 0) * 17 + 16; }
size_t besst_dev_reduce_workspace_bytes(int64_t n_tuples) { return reduce_workspace_bytes(n_tuples); }

int besst_dev_classify(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                       const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                       int64_t n_contigs, const void* contig_table, const besst_lib_params* p, int32_t node_bits,
                       int32_t* carry, int64_t* aligned, uint64_t* keys, uint64_t* payload, uint32_t* n_out,
                       besst_counters* counters, void* workspace, size_t workspace_bytes);

int besst_dev_reduce_flags(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits, const uint64_t* keys,
                           const uint64_t* payload, uint64_t* row_key, uint32_t* row_mask, uint32_t* row_n, int64_t* row_sum,
                           int64_t* row_sum_sq, uint32_t* row_first, uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi,
                           uint32_t* n_rows, void* workspace, size_t workspace_bytes, const uint32_t* first_map,
                           uint64_t key_base, uint32_t flags) {
    BESST_REQUIRE(n_tuples && n_rows, "reduce: null size pointer");
    BESST_REQUIRE(capacity == 0 || (keys && payload && row_key && row_mask && row_n && row_sum && row_sum_sq &&
                                    row_first && row_offset && obs_lo && obs_hi),
                  "reduce: null buffer");
    return launch_sort_reduce(static_cast<hipStream_t>(stream), capacity, n_tuples, key_bits, keys, payload, row_key,
                              row_mask, row_n, row_sum, row_sum_sq, row_first, row_offset, obs_lo, obs_hi, n_rows,
                              workspace, workspace_bytes, first_map, key_base, false, nullptr, flags);
}

int besst_dev_reduce(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits, const uint64_t* keys,
                     const uint64_t* payload, uint64_t* row_key, uint32_t* row_mask, uint32_t* row_n, int64_t* row_sum,
                     int64_t* row_sum_sq, uint32_t* row_first, uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi,
                     uint32_t* n_rows, void* workspace, size_t workspace_bytes, const uint32_t* first_map,
                     uint64_t key_base) {
    return besst_dev_reduce_flags(stream, capacity, n_tuples, key_bits, keys, payload, row_key, row_mask, row_n, row_sum,
                                  row_sum_sq, row_first, row_offset, obs_lo, obs_hi, n_rows, workspace, workspace_bytes,
                                  first_map, key_base, 0u);
}

int besst_dev_reduce_census(void* stream, int64_t capacity, int32_t key_bits, uint32_t flags, const void* workspace,
                            size_t workspace_bytes, int64_t* h_out) {
    return reduce_census(static_cast<hipStream_t>(stream), capacity, key_bits, flags, workspace, workspace_bytes, h_out);
}

static int fill_classify_args(ClassifyArgs& a, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                              const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                              int64_t n_contigs, const void* contig_table, const besst_lib_params* p,
                              int32_t node_bits) {
    BESST_REQUIRE(p, "classify: null params");
    BESST_REQUIRE(n >= 0, "classify: negative record count");
    BESST_REQUIRE(n == 0 || (tid && mtid && pos && mpos && flag && mapq && qlen), "classify: null column");
    BESST_REQUIRE(aligned16(tid) && aligned16(mtid) && aligned16(pos) && aligned16(mpos) && aligned16(flag) &&
                      aligned16(mapq) && aligned16(qlen),
                  "classify: record columns must be 16-byte aligned");
    BESST_REQUIRE(contig_table && aligned16(contig_table), "classify: contig table null or misaligned");
    BESST_REQUIRE(n_contigs > 0 && n_contigs < ((int64_t)1 << 31), "classify: n_contigs out of range");
    BESST_REQUIRE(node_bits >= 1 && node_bits <= 29, "classify: node_bits must be in [1, 29]");
    BESST_REQUIRE(p->orientation == 0 || p->orientation == 1, "classify: orientation must be 0 or 1");
    BESST_REQUIRE(p->ins_size_threshold < 1073741824.0, "classify: ins_size_threshold must be below 2^30");
    a.tid = tid; a.mtid = mtid; a.pos = pos; a.mpos = mpos; a.flag = flag; a.mapq = mapq; a.qlen = qlen;
    a.table = static_cast<const ContigRow*>(contig_table);
    a.cls8 = static_cast<const uint8_t*>(contig_table) + (size_t)n_contigs * sizeof(ContigRow);
    a.n = n;
    a.n_contigs = (int32_t)n_contigs;
    a.node_bits = node_bits;
    a.read_len = p->read_len;
    a.read_len_int = (p->read_len >= 0.0 && p->read_len < 2147483648.0 && p->read_len == floor(p->read_len)) ? (int64_t)p->read_len : -1;
    a.ins_size_threshold = p->ins_size_threshold;
    a.ins_thr_int = p->ins_size_threshold <= -4611686018427387904.0 ? INT64_MIN : (int64_t)ceil(p->ins_size_threshold);   // NaN and >= 2^30 were refused above
    a.min_mapq = p->min_mapq;
    a.rf = p->orientation;
    a.detect_dup = p->detect_duplicate;
    a.extend_paths = p->extend_paths;
    a.no_score = p->no_score;
    a.record_path = p->record_path;
    a.mate_bits = static_cast<const uint8_t*>(p->mate_bits);
    a.tid_bits = p->mate_bits ? static_cast<const uint8_t*>(p->tid_bits) : nullptr;   // (only honoured together)
    a.ps_table = nullptr; a.ps_rows = 0; a.ps_shift = 0; a.ps_base = 0;
    // the candidate side stream: only with both bit planes, only when made for this header and these records
    // (BESST_CAND_STREAM=0: never - A/B runs, tests)
    a.cs_off = nullptr; a.cs_set = nullptr; a.cs_tid = a.cs_mtid = a.cs_pos = a.cs_mpos = nullptr; a.cs_fq = nullptr; a.cs_mapq = nullptr;
    const char* cs_env = getenv("BESST_CAND_STREAM");
    const bool cs_knob = !(cs_env && cs_env[0] == '0' && cs_env[1] == 0);
    if (const besst_cand_stream* cs = p->cand_stream; cs && cs_knob && a.mate_bits && a.tid_bits && cs->n_refs == n_contigs &&
                                                      cs->n_records == n && n > 0) {
        BESST_REQUIRE(cs->offsets && cs->set_bits && cs->tid && cs->mtid && cs->pos && cs->mpos && cs->flag_qlen && cs->mapq,
                      "classify: candidate stream with a null member");
        a.cs_off = static_cast<const uint32_t*>(cs->offsets);
        a.cs_set = static_cast<const uint8_t*>(cs->set_bits);
        a.cs_tid = static_cast<const int32_t*>(cs->tid); a.cs_mtid = static_cast<const int32_t*>(cs->mtid);
        a.cs_pos = static_cast<const int32_t*>(cs->pos); a.cs_mpos = static_cast<const int32_t*>(cs->mpos);
        a.cs_fq = static_cast<const uint32_t*>(cs->flag_qlen);
        a.cs_mapq = static_cast<const uint8_t*>(cs->mapq);
    }
    BESST_REQUIRE(p->record_path == 0 || p->record_path == 1, "classify: record_path must be 0 or 1");
    return BESST_OK;
}

int besst_dev_classify(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                       const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                       int64_t n_contigs, const void* contig_table, const besst_lib_params* p, int32_t node_bits,
                       int32_t* carry, int64_t* aligned, uint64_t* keys, uint64_t* payload, uint32_t* n_out,
                       besst_counters* counters, void* workspace, size_t workspace_bytes) {
    ClassifyArgs a;
    int rc = fill_classify_args(a, n, tid, mtid, pos, mpos, flag, mapq, qlen, n_contigs, contig_table, p, node_bits);
    if (rc) return rc;
    BESST_REQUIRE(carry && aligned && keys && payload && n_out && counters, "classify: null output");
    return launch_classify(static_cast<hipStream_t>(stream), a, carry, aligned, keys, payload, n_out, counters,
                           workspace, workspace_bytes);
}

static void presort_to_spec(const besst_presort* h, PresortSpec& ps) {
    ps = PresortSpec{};
    if (!h || !h->table) return;
    ps.table = h->table; ps.rows = h->rows; ps.shift = h->shift; ps.key_base = h->key_base; ps.cap = h->capacity;
    ps.segmented = h->segmented; ps.in_record_loop = h->in_record_loop;
    // the run-grouped stage 2 (what a stream with this description takes unless the flag says otherwise) has no use for
    // the digit histograms: the record loop then does not count them
    ps.count = (runs_enabled((int64_t)h->capacity) && !(h->flags & BESST_REDUCE_NO_RUNS)) ? 0 : 1;
    ps.seg = SegSource{h->seg_keys, h->seg_payload, h->seg_offsets, h->seg_skip, h->seg_blocks, h->seg_tile, h->payload_out,
                       h->seg_chunk_first, h->seg_run_offsets, h->seg_summ, h->seg_summ_stride, h->seg_run_status};
}

int besst_dev_reduce_presort(int64_t capacity, int32_t key_bits, uint64_t key_base, void* workspace,
                             size_t workspace_bytes, besst_presort* h_out) {
    BESST_REQUIRE(h_out, "reduce_presort: null output");
    memset(h_out, 0, sizeof(*h_out));
    PresortSpec ps{};
    if (!sort_presort_spec(capacity, key_bits, key_base, workspace, workspace_bytes, &ps)) return 0;
    h_out->table = ps.table; h_out->rows = ps.rows; h_out->shift = ps.shift; h_out->key_base = ps.key_base;
    h_out->capacity = ps.cap;
    h_out->segmented = 1;            // every stream that takes the table can also be read from its block segments
    return 1;
}

int besst_dev_classify_presort(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                               const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                               int64_t n_contigs, const void* contig_table, const besst_lib_params* p, int32_t node_bits,
                               int32_t* carry, int64_t* aligned, uint64_t* keys, uint64_t* payload, uint32_t* n_out,
                               besst_counters* counters, void* workspace, size_t workspace_bytes,
                               besst_presort* h_presort) {
    ClassifyArgs a;
    int rc = fill_classify_args(a, n, tid, mtid, pos, mpos, flag, mapq, qlen, n_contigs, contig_table, p, node_bits);
    if (rc) return rc;
    BESST_REQUIRE(carry && aligned && keys && payload && n_out && counters, "classify: null output");
    PresortSpec ps;
    presort_to_spec(h_presort, ps);
    ps.in_record_loop = 0;
    rc = launch_classify(static_cast<hipStream_t>(stream), a, carry, aligned, keys, payload, n_out, counters,
                         workspace, workspace_bytes, ps.table ? &ps : nullptr);
    if (h_presort && h_presort->table) {
        h_presort->segmented = ps.segmented; h_presort->in_record_loop = ps.in_record_loop;
        h_presort->seg_keys = ps.seg.seg_keys; h_presort->seg_payload = ps.seg.seg_payload;
        h_presort->seg_offsets = ps.seg.offsets; h_presort->seg_skip = ps.seg.skip;
        h_presort->seg_blocks = ps.seg.nblocks; h_presort->seg_tile = ps.seg.tile; h_presort->payload_out = ps.seg.payload_out;
        h_presort->seg_chunk_first = ps.seg.chunk_first;
        h_presort->seg_run_offsets = ps.seg.run_offsets; h_presort->seg_summ = ps.seg.summ;
        h_presort->seg_summ_stride = ps.seg.summ_stride; h_presort->seg_run_status = ps.seg.run_status;
    }
    return rc;
}

int besst_dev_reduce_presorted(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t key_bits,
                               const uint64_t* keys, const uint64_t* payload, uint64_t* row_key, uint32_t* row_mask,
                               uint32_t* row_n, int64_t* row_sum, int64_t* row_sum_sq, uint32_t* row_first,
                               uint32_t* row_offset, int32_t* obs_lo, int32_t* obs_hi, uint32_t* n_rows,
                               void* workspace, size_t workspace_bytes, const uint32_t* first_map, uint64_t key_base,
                               const besst_presort* h_presort) {
    BESST_REQUIRE(n_tuples && n_rows, "reduce: null size pointer");
    BESST_REQUIRE(h_presort && h_presort->table, "reduce_presorted: no hand-over description");
    PresortSpec ps;
    presort_to_spec(h_presort, ps);
    const bool seg = ps.segmented != 0;
    BESST_REQUIRE(capacity == 0 || ((keys || seg) && payload && row_key && row_mask && row_n && row_sum && row_sum_sq &&
                                    row_first && row_offset && obs_lo && obs_hi),
                  "reduce: null buffer");
    BESST_REQUIRE(!seg || (ps.seg.seg_keys && ps.seg.seg_payload && ps.seg.offsets && ps.seg.skip &&
                           ps.seg.payload_out == payload && ps.seg.tile > 0),
                  "reduce_presorted: incomplete segment description");
    BESST_REQUIRE(h_presort->in_record_loop != 3 || (seg && ps.seg.run_offsets && ps.seg.summ && ps.seg.run_status),
                  "reduce_presorted: incomplete description of the record loop's runs");
    if (h_presort->in_record_loop >= 2 && (h_presort->flags & BESST_REDUCE_NO_RUNS)) {
        set_error("reduce_presorted: the classify call behind this description did not count the sort's digits (its flags "
                  "asked for the run-grouped form): repeat it with BESST_REDUCE_NO_RUNS in `flags`");
        return BESST_ERR_STATE;
    }
    return launch_sort_reduce(static_cast<hipStream_t>(stream), capacity, n_tuples, key_bits, keys, payload, row_key,
                              row_mask, row_n, row_sum, row_sum_sq, row_first, row_offset, obs_lo, obs_hi, n_rows,
                              workspace, workspace_bytes, first_map, key_base, true, seg ? &ps.seg : nullptr,
                              h_presort->flags);
}

int besst_dev_candidate_density(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid,
                                int64_t sample_records, void* counts_scratch, double* h_share,
                                int32_t* h_record_path) {
    BESST_REQUIRE(n >= 0 && (n == 0 || (tid && mtid)) && counts_scratch && h_share && h_record_path,
                  "candidate_density: bad argument");
    unsigned long long host[2] = {0ull, 0ull};
    if (n > 0) {
        int rc = launch_candidate_density(static_cast<hipStream_t>(stream), n, tid, mtid, sample_records,
                                          static_cast<unsigned long long*>(counts_scratch));
        if (rc) return rc;
        BESST_HIP_TRY(hipMemcpyAsync(host, counts_scratch, sizeof(host), hipMemcpyDeviceToHost,
                                     static_cast<hipStream_t>(stream)));
        BESST_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    }
    *h_share = host[1] ? (double)host[0] / (double)host[1] : 0.0;
    *h_record_path = *h_share >= BESST_DENSE_CANDIDATE_SHARE ? 1 : 0;
    return BESST_OK;
}

int besst_dev_classify_scan(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* pos,
                            const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq, const uint16_t* qlen,
                            int64_t n_contigs, const void* contig_table, const besst_lib_params* p, int32_t node_bits,
                            int64_t* aligned, besst_counters* counters, void* workspace, size_t workspace_bytes) {
    ClassifyArgs a;
    int rc = fill_classify_args(a, n, tid, mtid, pos, mpos, flag, mapq, qlen, n_contigs, contig_table, p, node_bits);
    if (rc) return rc;
    BESST_REQUIRE(aligned && counters, "classify_scan: null output");
    return launch_classify_scan(static_cast<hipStream_t>(stream), a, aligned, counters, workspace, workspace_bytes);
}

int besst_dev_classify_tail(void* stream, int64_t n, int32_t* tail, void* workspace, size_t workspace_bytes) {
    BESST_REQUIRE(tail, "classify_tail: null output");
    return launch_classify_tail(static_cast<hipStream_t>(stream), n, tail, workspace, workspace_bytes);
}

int besst_dev_resolve_carry(void* stream, const int32_t* tails, int32_t rank, int32_t* carry) {
    BESST_REQUIRE(tails && carry && rank >= 0, "resolve_carry: bad argument");
    return launch_resolve_carry(static_cast<hipStream_t>(stream), tails, rank, carry);
}

int besst_dev_classify_emit(void* stream, int64_t n, int32_t detect_duplicate, int32_t* carry, uint64_t* keys,
                            uint64_t* payload, uint32_t* n_out, besst_counters* counters, void* workspace,
                            size_t workspace_bytes, int64_t n_contigs, const void* contig_table, int64_t* aligned,
                            const int32_t* tails, int32_t rank, int32_t* slice_info) {
    BESST_REQUIRE(!(tails && slice_info), "classify_emit: tails and slice_info exclude each other");
    BESST_REQUIRE(carry && keys && payload && n_out && counters && contig_table && aligned,
                  "classify_emit: null pointer");
    BESST_REQUIRE(n_contigs > 0 && n_contigs < ((int64_t)1 << 31), "classify_emit: n_contigs out of range");
    BESST_REQUIRE(rank >= 0 && rank <= 65536, "classify_emit: rank out of range");
    const uint8_t* cls8 = static_cast<const uint8_t*>(contig_table) + (size_t)n_contigs * sizeof(ContigRow);
    return launch_classify_emit(static_cast<hipStream_t>(stream), n, detect_duplicate, carry, keys, payload, n_out,
                                counters, workspace, workspace_bytes, cls8, (int32_t)n_contigs, aligned, tails, rank,
                                slice_info);
}

size_t besst_dev_exchange_region_bytes(int64_t pair_capacity) { return exchange_region_bytes(pair_capacity); }
size_t besst_dev_exchange_stride_bytes(int64_t pair_capacity, int64_t rider_bytes) {
    return exchange_stride_bytes(pair_capacity, rider_bytes < 0 ? 0 : rider_bytes);
}

uint32_t besst_owner_of_scaffold(uint32_t scaffold_id, uint32_t world) { return owner_of_scaffold(scaffold_id, world ? world : 1); }

int besst_dev_partition(void* stream, int64_t capacity, const uint32_t* n_tuples, int32_t node_bits, int32_t world,
                        const uint64_t* keys, const uint64_t* payload, int64_t pair_capacity, void* send_buffer,
                        void* workspace, size_t workspace_bytes, const void* rider, int64_t rider_bytes,
                        const int32_t* slice_info) {
    BESST_REQUIRE(n_tuples && keys && payload && send_buffer, "partition: null pointer");
    return launch_partition(static_cast<hipStream_t>(stream), capacity, n_tuples, node_bits, world, keys, payload,
                            pair_capacity, send_buffer, workspace, workspace_bytes, rider, rider_bytes, slice_info);
}

int besst_dev_unpack(void* stream, int32_t world, int64_t pair_capacity, const void* recv_buffer, uint64_t* keys,
                     uint64_t* payload, uint32_t* gidx, uint32_t* n_out, uint32_t* overflow, void* rider_sum,
                     int64_t rider_bytes, int32_t speculative_heads, int32_t rank, int32_t detect_duplicate,
                     int32_t* all_slice_info, besst_counters* counters) {
    BESST_REQUIRE(recv_buffer && keys && payload && gidx && n_out && overflow, "unpack: null pointer");
    return launch_unpack(static_cast<hipStream_t>(stream), world, pair_capacity, recv_buffer, keys, payload, gidx,
                         n_out, overflow, rider_sum, rider_bytes, speculative_heads, rank, detect_duplicate,
                         all_slice_info, counters);
}

int besst_dev_score_edges(void* stream, int64_t n_edges, const uint32_t* row, const uint8_t* swap, const int32_t* len1,
                          const int32_t* len2, const uint32_t* row_n, const int64_t* row_sum, const uint32_t* row_offset,
                          const int32_t* obs_lo, const int32_t* obs_hi, double mean, double sigma, double read_len,
                          double* gap, double* sd0, int32_t* ks_h, uint8_t* flags, void* workspace,
                          size_t workspace_bytes) {
    BESST_REQUIRE(n_edges >= 0 && n_edges < ((int64_t)1 << 31), "dev_score_edges: edge count out of range");
    if (n_edges == 0) return BESST_OK;
    BESST_REQUIRE(row && swap && len1 && len2 && row_n && row_sum && row_offset && obs_lo && obs_hi && gap && sd0 &&
                      ks_h && flags && workspace,
                  "dev_score_edges: null pointer");
    BESST_REQUIRE(sigma > 0.0, "dev_score_edges: sigma must be positive");
    BESST_REQUIRE(workspace_bytes >= align_up((size_t)n_edges * 8, 256), "dev_score_edges: workspace too small");
    ScoreArgs a;
    a.row = row; a.swap = swap; a.len1 = len1; a.len2 = len2;
    a.row_n = row_n; a.row_sum = row_sum; a.row_offset = row_offset;
    a.obs_lo = obs_lo; a.obs_hi = obs_hi;
    a.mean = mean; a.sigma = sigma; a.read_len = read_len;
    a.n_edges = n_edges;
    return launch_score(static_cast<hipStream_t>(stream), a, gap, sd0, ks_h, flags, workspace, workspace_bytes);
}

int besst_dev_score_edges_lognormal(void* stream, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                                    const int32_t* len1, const int32_t* len2, const uint32_t* row_n, const int64_t* row_sum,
                                    const uint32_t* row_offset, const int32_t* obs_lo, const int32_t* obs_hi, double mean,
                                    double sigma, double read_len, double ln_mu, double ln_sigma, int64_t x_max,
                                    const double* F0, const double* F1, int32_t max_gap, double* gap, int32_t* ks_h,
                                    uint8_t* flags, void* workspace, size_t workspace_bytes) {
    BESST_REQUIRE(n_edges >= 0 && n_edges < ((int64_t)1 << 31), "dev_score_edges_lognormal: edge count out of range");
    if (n_edges == 0) return BESST_OK;
    BESST_REQUIRE(row && swap && len1 && len2 && row_n && row_sum && row_offset && obs_lo && obs_hi && gap && ks_h &&
                      flags && workspace && F0 && F1,
                  "dev_score_edges_lognormal: null pointer");
    BESST_REQUIRE(sigma > 0.0 && ln_sigma > 0.0 && x_max >= 1 && max_gap >= 0, "dev_score_edges_lognormal: parameters out of range");
    // [ big_off | sort scratch | tail tables G0, G1 and the workspace that builds them | sd0 (unused by the caller: the
    //   conditional sigma is looked up with the gap) ]
    const size_t head = align_up((size_t)n_edges * 8, 256);
    const size_t tails = lognormal_dev_tails_bytes(x_max);
    BESST_REQUIRE(workspace_bytes >= 2 * head + tails, "dev_score_edges_lognormal: workspace too small");
    ScoreArgs a;
    a.row = row; a.swap = swap; a.len1 = len1; a.len2 = len2;
    a.row_n = row_n; a.row_sum = row_sum; a.row_offset = row_offset;
    a.obs_lo = obs_lo; a.obs_hi = obs_hi;
    a.mean = mean; a.sigma = sigma; a.read_len = read_len;
    a.n_edges = n_edges;
    // the kernel wants the sort scratch right behind the offsets: the tail tables and the sd0 column sit at the END
    char* const end = static_cast<char*>(workspace) + workspace_bytes;
    auto* sd0 = reinterpret_cast<double*>(end - head);
    const size_t tab = align_up((size_t)(x_max + 1) * 8, 256);
    auto* G0 = reinterpret_cast<double*>(end - head - tails);
    auto* G1 = reinterpret_cast<double*>(end - head - tails + tab);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = launch_lognormal_tails(s, ln_mu, ln_sigma, x_max, G0, G1, end - head - tails + 2 * tab, tails - 2 * tab);
    if (rc) return rc;
    LogNormalArgs l{ln_mu, ln_sigma, x_max, F0, F1, max_gap, G0, G1};
    return launch_score_lognormal(s, a, l, gap, sd0, ks_h, flags, workspace, workspace_bytes - head - tails);
}

size_t besst_dev_mate_bits_bytes(int64_t n_records) { return (size_t)(((n_records > 0 ? n_records : 0) + 7) / 8) + 16; }

int besst_dev_mate_bits(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, void* bits) {
    BESST_REQUIRE(n >= 0, "dev_mate_bits: negative record count");
    if (n == 0) return BESST_OK;
    BESST_REQUIRE(tid && mtid && bits, "dev_mate_bits: null pointer");
    BESST_REQUIRE(aligned16(tid) && aligned16(mtid), "dev_mate_bits: columns must be 16-byte aligned");
    return launch_mate_bits(static_cast<hipStream_t>(stream), tid, mtid, 0, n, n, static_cast<uint8_t*>(bits), nullptr);
}

int besst_dev_record_bits(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, void* mate_bits, void* tid_bits) {
    BESST_REQUIRE(n >= 0, "dev_record_bits: negative record count");
    if (n == 0) return BESST_OK;
    BESST_REQUIRE(tid && mtid && mate_bits && tid_bits, "dev_record_bits: null pointer");
    BESST_REQUIRE(aligned16(tid) && aligned16(mtid), "dev_record_bits: columns must be 16-byte aligned");
    return launch_mate_bits(static_cast<hipStream_t>(stream), tid, mtid, 0, n, n, static_cast<uint8_t*>(mate_bits),
                            static_cast<uint8_t*>(tid_bits));
}

// ---- the candidate side stream: entries per column rounded up past n_entries (the loop's idle lanes read one more)
static size_t cand_stream_cap(int64_t n_entries) { return align_up((size_t)(n_entries > 0 ? n_entries : 0) + 1, 64); }

size_t besst_dev_candidate_offsets_bytes(int64_t n_records) {
    const int64_t n = n_records > 0 ? n_records : 0;
    return align_up((size_t)((n + kClsTile - 1) / kClsTile + 1) * sizeof(uint32_t), 16);
}

size_t besst_dev_candidate_stream_bytes(int64_t n_entries) { return cand_stream_cap(n_entries) * 21; }

int besst_dev_candidate_offsets(void* stream, int64_t n, int64_t n_refs, const int32_t* tid, const int32_t* mtid,
                                const uint16_t* flag, void* set_bits, void* offsets, void* mate_bits, void* tid_bits) {
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), "dev_candidate_offsets: record count out of range");
    BESST_REQUIRE(n_refs >= 0, "dev_candidate_offsets: negative reference count");
    BESST_REQUIRE(offsets && (n == 0 || (tid && mtid && flag && set_bits)), "dev_candidate_offsets: null pointer");
    BESST_REQUIRE((mate_bits == nullptr) == (tid_bits == nullptr), "dev_candidate_offsets: both bit planes or neither");
    BESST_REQUIRE(aligned16(tid) && aligned16(mtid) && aligned16(flag) && aligned16(set_bits),
                  "dev_candidate_offsets: columns and the set plane must be 16-byte aligned");
    return launch_cand_offsets(static_cast<hipStream_t>(stream), n, n_refs, tid, mtid, flag, static_cast<uint8_t*>(set_bits),
                               static_cast<uint32_t*>(offsets), static_cast<uint8_t*>(mate_bits), static_cast<uint8_t*>(tid_bits));
}

int besst_dev_candidate_stream(void* stream, int64_t n, int64_t n_refs, const int32_t* tid, const int32_t* mtid,
                               const int32_t* pos, const int32_t* mpos, const uint16_t* flag, const uint8_t* mapq,
                               const uint16_t* qlen, const void* set_bits, const void* offsets, int64_t n_entries,
                               void* entries, size_t entries_bytes, besst_cand_stream* out) {
    BESST_REQUIRE(out, "dev_candidate_stream: null descriptor");
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 32) && n_entries >= 0 && n_entries <= n, "dev_candidate_stream: counts out of range");
    BESST_REQUIRE(offsets && entries && (n == 0 || (tid && mtid && pos && mpos && flag && mapq && qlen && set_bits)),
                  "dev_candidate_stream: null pointer");
    BESST_REQUIRE(aligned16(set_bits) && aligned16(entries), "dev_candidate_stream: the set plane and the entries must be 16-byte aligned");
    BESST_REQUIRE(entries_bytes >= besst_dev_candidate_stream_bytes(n_entries), "dev_candidate_stream: entry buffer too small");
    const size_t cap = cand_stream_cap(n_entries);
    char* p = static_cast<char*>(entries);
    auto* e_tid = reinterpret_cast<int32_t*>(p), *e_mtid = reinterpret_cast<int32_t*>(p + cap * 4);
    auto* e_pos = reinterpret_cast<int32_t*>(p + cap * 8), *e_mpos = reinterpret_cast<int32_t*>(p + cap * 12);
    auto* e_fq = reinterpret_cast<uint32_t*>(p + cap * 16);
    auto* e_mapq = reinterpret_cast<uint8_t*>(p + cap * 20);
    *out = besst_cand_stream{n_refs, n, n_entries, offsets, set_bits, e_tid, e_mtid, e_pos, e_mpos, e_fq, e_mapq};
    return launch_cand_entries(static_cast<hipStream_t>(stream), n, tid, mtid, pos, mpos, flag, mapq, qlen,
                               static_cast<const uint8_t*>(set_bits), static_cast<const uint32_t*>(offsets), e_tid, e_mtid,
                               e_pos, e_mpos, e_fq, e_mapq, (uint32_t)(cap > 0xffffffffull ? 0xffffffffull : cap));
}

int besst_dev_record_loop_form(void) { return classify_last_form(); }

size_t besst_dev_lognormal_tables_workspace_bytes(int64_t x_max) { return lognormal_tables_workspace_bytes(x_max); }

int besst_dev_lognormal_tables(void* stream, double mu, double sigma, int64_t x_max, double* F0, double* F1, void* workspace,
                               size_t workspace_bytes) {
    return launch_lognormal_tables(static_cast<hipStream_t>(stream), mu, sigma, x_max, F0, F1, workspace, workspace_bytes);
}

int besst_dev_conditional_stddevs(void* stream, const double* density, int64_t max_isize, const int32_t* steps,
                                  int32_t n_steps, double* out) {
    BESST_REQUIRE(n_steps >= 0, "dev_conditional_stddevs: negative step count");
    return launch_conditional_stddevs(static_cast<hipStream_t>(stream), density, max_isize, steps, n_steps, out);
}

size_t besst_dev_metrics_workspace_bytes(int64_t n_records) { return metrics_workspace_bytes(n_records < 1 ? 1 : n_records); }

int besst_dev_metrics_sample(void* stream, int64_t n, const int32_t* tid, const int32_t* mtid, const int32_t* tlen,
                             const uint16_t* flag, const uint8_t* mapq, int64_t n_contigs, const uint8_t* top_mask,
                             int32_t orientation, int32_t min_mapq, double read_len, int32_t count_only,
                             int32_t* isize_out, int32_t* contam_out, int64_t* state, void* workspace,
                             size_t workspace_bytes) {
    // (every record index in metrics.hip is 64 bits wide and the sampling form works in parts of 64 Mi records; the bound is
    // what the count-only form's one launch of n / 4096 workgroups and their uint32 counts were checked for)
    BESST_REQUIRE(n >= 0 && n < ((int64_t)1 << 36), "dev_metrics_sample: n out of range");
    BESST_REQUIRE(n_contigs > 0 && n_contigs < ((int64_t)1 << 31), "dev_metrics_sample: n_contigs out of range");
    BESST_REQUIRE(orientation == 0 || orientation == 1, "dev_metrics_sample: orientation must be 0 or 1");
    BESST_REQUIRE(state && top_mask, "dev_metrics_sample: null pointer");
    BESST_REQUIRE(count_only || contam_out, "dev_metrics_sample: contam_out is null");
    BESST_REQUIRE(n == 0 || (tid && mtid && tlen && flag && mapq), "dev_metrics_sample: null column");
    MetricsArgs a;
    a.tid = tid; a.mtid = mtid; a.tlen = tlen; a.flag = flag; a.mapq = mapq;
    a.top_mask = top_mask;
    a.n = n;
    a.n_contigs = (int32_t)n_contigs;
    a.rf = orientation;
    a.min_mapq = min_mapq;
    a.read_len = read_len;
    return launch_metrics(static_cast<hipStream_t>(stream), a, 0, n, isize_out, contam_out, state, workspace,
                          workspace_bytes, count_only != 0);
}

int besst_ctx_build_graph(besst_ctx* c) {
    BESST_REQUIRE(c, "null context");
    if (!c->have_lib || c->n_contigs <= 0) {
        set_error("build_graph: set_contigs and set_library must be called first");
        return BESST_ERR_STATE;
    }
    int rc = use_device(c);
    if (rc) return rc;
    const int64_t n = c->n_records;
    auto* sb = reinterpret_cast<SmallBlock*>(c->small.p);
    SmallBlock init;
    memset(&init, 0, sizeof(init));
    init.carry[0] = -1;   // counters(0, 0, 0, 0, -1, -1, 0): CreateGraph.py:98
    init.carry[1] = -1;
    BESST_HIP_TRY(hipMemcpyAsync(sb, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemsetAsync(c->aligned.p, 0, (size_t)c->n_contigs * sizeof(int64_t), c->stream));
    const size_t cap1 = (size_t)(n > 0 ? n : 1);
    if ((rc = c->keys.ensure(cap1))) return rc;
    if ((rc = c->payload.ensure(cap1))) return rc;
    if ((rc = c->ws.ensure(classify_workspace_bytes(n)))) return rc;
    besst_lib_params lp = c->lib;
    {   // which form of the record loop: one fused pass for candidate-dense (mate-pair) libraries
        double share = 0.0;
        if ((rc = c->aux.ensure(64))) return rc;
        rc = besst_dev_candidate_density(c->stream, n, c->tid.p, c->mtid.p, 4 << 20, c->aux.p, &share, &lp.record_path);
        if (rc) return rc;
        const char* forced = getenv("BESST_RECORD_PATH");   // tests and experiments: "0" / "1"
        if (forced && (forced[0] == '0' || forced[0] == '1') && forced[1] == 0) lp.record_path = forced[0] - '0';
    }
    {   // the mate-elsewhere bits of the records that have none yet (everything pushed since the last build): 8 bytes read
        // per record once, after which every pass over these records leaves `mtid` alone where tid == mtid.
        // BESST_MATE_BITS=0 (tests): the loop compares the columns itself.
        // The run bits (record i lies on another reference than record i - 1) are made in the same pass and extended with
        // them: a push's first record is compared with the resident record before it.  BESST_TID_BITS=0: only the mate
        // bits, the fused loop reads `tid` of every record.
        const char* off = getenv("BESST_MATE_BITS");
        const char* tid_off = getenv("BESST_TID_BITS");
        lp.mate_bits = nullptr;
        lp.tid_bits = nullptr;
        lp.cand_stream = nullptr;                            // (a stream describes the caller's columns, never the context's own)
        if (!(off && off[0] == '0' && off[1] == 0) && n > 0) {
            const bool runs = !(tid_off && tid_off[0] == '0' && tid_off[1] == 0);
            const size_t need = (size_t)((n + 7) / 8) + 16;
            if (need > c->mate_bits.cap) {                   // (growing drops what was there)
                if ((rc = c->mate_bits.ensure(need + need / 2))) return rc;
                c->bits_upto = 0;
            }
            if (runs && need > c->tid_bits.cap) {
                if ((rc = c->tid_bits.ensure(need + need / 2))) return rc;
                c->tid_bits_upto = 0;
            }
            // (one launch writes both planes from the shorter of the two: they differ only after a build without run bits)
            const int64_t upto = runs && c->tid_bits_upto < c->bits_upto ? c->tid_bits_upto : c->bits_upto;
            if (upto < n) {
                if ((rc = launch_mate_bits(c->stream, c->tid.p, c->mtid.p, upto, n, n, c->mate_bits.p,
                                           runs ? c->tid_bits.p : nullptr)))
                    return rc;
                ++c->maker_launches;
                c->bits_upto = n;
                if (runs) c->tid_bits_upto = n;
            }
            lp.mate_bits = c->mate_bits.p;
            if (runs) lp.tid_bits = c->tid_bits.p;
            // The candidate side stream (fused loop only), extended like the planes for what was pushed since the last
            // build: the block that was the stream's last then - a push may have ended inside it - is counted and written
            // again whole, its entries go on where that block's began.  A buffer that has to grow drops what was there,
            // and so does a contig table of another size (the set rule reads n_refs).  BESST_CAND_STREAM=0: no stream.
            const char* cs_off_env = getenv("BESST_CAND_STREAM");
            if (runs && lp.record_path == 1 && !(cs_off_env && cs_off_env[0] == '0' && cs_off_env[1] == 0)) {
                if (c->cs.n_refs != c->n_contigs) c->cs_upto = 0;
                const size_t off_words = besst_dev_candidate_offsets_bytes(n) / sizeof(uint32_t);
                if (need > c->cs_set.cap) {
                    if ((rc = c->cs_set.ensure(need + need / 2))) return rc;
                    c->cs_upto = 0;
                }
                if (off_words > c->cs_off.cap) {
                    if ((rc = c->cs_off.ensure(off_words + off_words / 2))) return rc;
                    c->cs_upto = 0;
                }
                if (c->cs_upto < n) {
                    const uint32_t nblocks = (uint32_t)((n + kClsTile - 1) / kClsTile);
                    uint32_t first = (uint32_t)(c->cs_upto / kClsTile);
                    if ((rc = launch_cand_offsets(c->stream, n, c->n_contigs, c->tid.p, c->mtid.p, c->flag.p, c->cs_set.p, c->cs_off.p,
                                                  nullptr, nullptr, first)))
                        return rc;
                    ++c->maker_launches;
                    uint32_t total = 0;
                    BESST_HIP_TRY(hipMemcpyAsync(&total, c->cs_off.p + nblocks, sizeof(total), hipMemcpyDeviceToHost, c->stream));
                    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
                    // (the columns lie one behind the other at a stride the capacity sets: more entries than the buffer was
                    // carved for move every column, so the entries are written again from the first block; the idle lanes
                    // of the loop read one entry behind the last)
                    if ((int64_t)total + 1 > c->cs_cap_entries) {
                        const size_t bytes = besst_dev_candidate_stream_bytes(total);
                        if ((rc = c->cs_entries.ensure(bytes + bytes / 2))) return rc;
                        c->cs_cap_entries = (int64_t)(c->cs_entries.cap / 21 / 64 * 64);
                        first = 0;
                    }
                    const size_t cap = (size_t)c->cs_cap_entries;
                    char* e = reinterpret_cast<char*>(c->cs_entries.p);
                    c->cs = besst_cand_stream{c->n_contigs, n, (int64_t)total, c->cs_off.p, c->cs_set.p, e, e + cap * 4, e + cap * 8,
                                              e + cap * 12, e + cap * 16, e + cap * 20};
                    if ((rc = launch_cand_entries(c->stream, n, c->tid.p, c->mtid.p, c->pos.p, c->mpos.p, c->flag.p, c->mapq.p,
                                                  c->qlen.p, c->cs_set.p, c->cs_off.p, reinterpret_cast<int32_t*>(e),
                                                  reinterpret_cast<int32_t*>(e + cap * 4), reinterpret_cast<int32_t*>(e + cap * 8),
                                                  reinterpret_cast<int32_t*>(e + cap * 12), reinterpret_cast<uint32_t*>(e + cap * 16),
                                                  reinterpret_cast<uint8_t*>(e + cap * 20), (uint32_t)cap, first)))
                        return rc;
                    ++c->maker_launches;
                    c->cs_upto = n;
                }
                c->cs.n_records = n;
                lp.cand_stream = &c->cs;
            }
        }
    }
    rc = besst_dev_classify(c->stream, n, c->tid.p, c->mtid.p, c->pos.p, c->mpos.p, c->flag.p, c->mapq.p, c->qlen.p,
                            c->n_contigs, c->table.p, &lp, c->node_bits, sb->carry, c->aligned.p, c->keys.p,
                            c->payload.p, &sb->n_out, &sb->counters, c->ws.p, c->ws.cap);
    if (rc) return rc;
    SmallBlock host;
    BESST_HIP_TRY(hipMemcpyAsync(&host, sb, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t L = host.n_out;
    c->n_tuples = L;
    const size_t cap2 = (size_t)(L > 0 ? L : 1);
    if ((rc = c->row_key.ensure(cap2))) return rc;
    if ((rc = c->row_mask.ensure(cap2))) return rc;
    if ((rc = c->row_n.ensure(cap2))) return rc;
    if ((rc = c->row_first.ensure(cap2))) return rc;
    if ((rc = c->row_offset.ensure(cap2))) return rc;
    if ((rc = c->row_sum.ensure(cap2))) return rc;
    if ((rc = c->row_sum_sq.ensure(cap2))) return rc;
    if ((rc = c->obs_lo.ensure(cap2))) return rc;
    if ((rc = c->obs_hi.ensure(cap2))) return rc;
    if ((rc = c->ws.ensure(reduce_workspace_bytes(L)))) return rc;
    // large streams take the run-grouped form first; one whose keys do not cluster says so in n_rows and is sorted
    // tuple by tuple instead (include/besst_amd.h, BESST_ROWS_*)
    for (uint32_t flags = 0;; flags = BESST_REDUCE_NO_RUNS) {
        rc = besst_dev_reduce_flags(c->stream, L, &sb->n_out, c->key_bits, c->keys.p, c->payload.p, c->row_key.p,
                                    c->row_mask.p, c->row_n.p, c->row_sum.p, c->row_sum_sq.p, c->row_first.p,
                                    c->row_offset.p, c->obs_lo.p, c->obs_hi.p, &sb->n_rows, c->ws.p, c->ws.cap, nullptr,
                                    c->key_base, flags);
        if (rc) return rc;
        BESST_HIP_TRY(hipMemcpyAsync(&host, sb, sizeof(host), hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
        if (host.n_rows == BESST_ROWS_RUN_OVERFLOW && flags == 0) continue;
        break;
    }
    if (host.n_rows == BESST_ROWS_SORT_FAILED || host.n_rows == BESST_ROWS_RUN_OVERFLOW) {
        set_error("build_graph: the sort could not finish (status word 0x%08x): a chained-scan look-back gave up", host.n_rows);
        return BESST_ERR_HIP;
    }
    c->n_rows = host.n_rows;
    c->built = true;
    return BESST_OK;
}

#define BESST_NEED_BUILT(c)                                                   \
    do {                                                                      \
        BESST_REQUIRE(c, "null context");                                     \
        if (!(c)->built) {                                                    \
            set_error("no edge table: call besst_ctx_build_graph first");     \
            return BESST_ERR_STATE;                                           \
        }                                                                     \
    } while (0)

int besst_ctx_edge_count(besst_ctx* c, int64_t* n_rows, int64_t* n_tuples) {
    BESST_NEED_BUILT(c);
    if (n_rows) *n_rows = c->n_rows;
    if (n_tuples) *n_tuples = c->n_tuples;
    return BESST_OK;
}

int besst_ctx_fetch_edges(besst_ctx* c, uint64_t* key, uint32_t* mask, uint32_t* n, int64_t* sum_obs,
                          int64_t* sum_obs_sq, uint32_t* first_idx, uint32_t* offset, int32_t* node_bits) {
    BESST_NEED_BUILT(c);
    int rc = use_device(c);
    if (rc) return rc;
    const size_t r = (size_t)c->n_rows;
    if (node_bits) *node_bits = c->node_bits;
    if (r) {
        BESST_REQUIRE(key && mask && n && sum_obs && sum_obs_sq && first_idx && offset, "fetch_edges: null buffer");
        BESST_HIP_TRY(hipMemcpyAsync(key, c->row_key.p, r * 8, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(mask, c->row_mask.p, r * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(n, c->row_n.p, r * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(sum_obs, c->row_sum.p, r * 8, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(sum_obs_sq, c->row_sum_sq.p, r * 8, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(first_idx, c->row_first.p, r * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(offset, c->row_offset.p, r * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return BESST_OK;
}

int besst_ctx_fetch_observations(besst_ctx* c, int32_t* obs_lo, int32_t* obs_hi) {
    BESST_NEED_BUILT(c);
    int rc = use_device(c);
    if (rc) return rc;
    const size_t L = (size_t)c->n_tuples;
    if (L) {
        BESST_REQUIRE(obs_lo && obs_hi, "fetch_observations: null buffer");
        BESST_HIP_TRY(hipMemcpyAsync(obs_lo, c->obs_lo.p, L * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipMemcpyAsync(obs_hi, c->obs_hi.p, L * 4, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return BESST_OK;
}

namespace {
__global__ __launch_bounds__(256) void obs_sum_kernel(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int32_t* __restrict__ out,
                                                      long long n) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = lo[i] + hi[i];
}
}  // namespace

// One observation per link (obs1 + obs2: what the reference keeps in an edge's 'observations', CreateGraph.py:849,862),
// summed on the device and copied on a stream of the context's own: the ONE call of the ctx layer that may run on a second
// host thread beside the calling thread's (score_edges, the fetches): it touches nothing those use but reads obs_lo / obs_hi.
int besst_ctx_fetch_observation_sums(besst_ctx* c, int32_t* out) {
    BESST_NEED_BUILT(c);
    if (hipSetDevice(c->device) != hipSuccess) { set_error("fetch_observation_sums: cannot select device %d", c->device); return BESST_ERR_HIP; }
    const int64_t L = c->n_tuples;
    if (L <= 0) return BESST_OK;
    BESST_REQUIRE(out, "fetch_observation_sums: null buffer");
    if (!c->side_stream) BESST_HIP_TRY(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    int rc = c->obs_sum.ensure((size_t)L);
    if (rc) return rc;
    const int64_t want = (L + 1023) / 1024;
    hipLaunchKernelGGL(obs_sum_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, c->side_stream, c->obs_lo.p, c->obs_hi.p,
                       c->obs_sum.p, (long long)L);
    BESST_HIP_TRY(hipGetLastError());
    BESST_HIP_TRY(hipMemcpyAsync(out, c->obs_sum.p, (size_t)L * 4, hipMemcpyDeviceToHost, c->side_stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->side_stream));
    return BESST_OK;
}

int besst_ctx_fetch_coverage(besst_ctx* c, int64_t* aligned) {
    BESST_NEED_BUILT(c);
    BESST_REQUIRE(aligned, "fetch_coverage: null buffer");
    int rc = use_device(c);
    if (rc) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(aligned, c->aligned.p, (size_t)c->n_contigs * 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int besst_ctx_fetch_counters(besst_ctx* c, besst_counters* out) {
    BESST_NEED_BUILT(c);
    BESST_REQUIRE(out, "fetch_counters: null buffer");
    int rc = use_device(c);
    if (rc) return rc;
    SmallBlock host;
    BESST_HIP_TRY(hipMemcpyAsync(&host, c->small.p, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    *out = host.counters;
    out->prev_obs1 = host.carry[0];
    out->prev_obs2 = host.carry[1];
    return BESST_OK;
}

}  // extern "C"

extern "C" {

int besst_dev_stream_order(void* stream, int64_t n, const int32_t* tid, const int32_t* pos, int64_t* first_unsorted) {
    BESST_REQUIRE(n >= 0 && first_unsorted && (n == 0 || (tid && pos)), "dev_stream_order: null pointer or negative count");
    hipStream_t s = static_cast<hipStream_t>(stream);
    BESST_HIP_TRY(hipMemsetAsync(first_unsorted, 0xff, sizeof(int64_t), s));     // -1: sorted
    return launch_stream_order(s, tid, pos, n, reinterpret_cast<unsigned long long*>(first_unsorted));
}

int besst_ctx_stream_order(besst_ctx* c, int64_t* first_unsorted, int32_t* first_key, int32_t* last_key) {
    BESST_REQUIRE(c && first_unsorted, "stream_order: null pointer");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = c->aux.ensure(64))) return rc;
    int64_t* word = reinterpret_cast<int64_t*>(c->aux.p);
    if ((rc = besst_dev_stream_order(c->stream, c->n_records, c->tid.p, c->pos.p, word))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(first_unsorted, word, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    // (tid, pos) of the first and the last resident record: what a slice of a sharded stream compares with its neighbours
    const int64_t n = c->n_records;
    if (first_key) {
        first_key[0] = first_key[1] = 0;
        if (n > 0) {
            BESST_HIP_TRY(hipMemcpyAsync(first_key, c->tid.p, 4, hipMemcpyDeviceToHost, c->stream));
            BESST_HIP_TRY(hipMemcpyAsync(first_key + 1, c->pos.p, 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (last_key) {
        last_key[0] = last_key[1] = 0;
        if (n > 0) {
            BESST_HIP_TRY(hipMemcpyAsync(last_key, c->tid.p + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
            BESST_HIP_TRY(hipMemcpyAsync(last_key + 1, c->pos.p + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int64_t besst_dev_library_report_words(int64_t n_refs, int64_t isize_bins) {
    if (n_refs < 0 || n_refs >= ((int64_t)1 << 31) || isize_bins < 1 || isize_bins > BESST_REPORT_MAX_ISIZE_BINS) return 0;
    return (int64_t)BESST_REPORT_REFS + 2 * n_refs + 3 * (isize_bins + 1);
}

int besst_dev_library_report(void* stream, const besst_report_args* a, uint64_t* out) {
    BESST_REQUIRE(a && out, "dev_library_report: null pointer");
    BESST_REQUIRE(a->n_records >= 0 && a->n_records < ((int64_t)1 << 32), "dev_library_report: n_records out of range");
    BESST_REQUIRE(a->n_refs >= 0 && a->n_refs < ((int64_t)1 << 31), "dev_library_report: n_refs out of range");
    BESST_REQUIRE(a->isize_bins >= 1 && a->isize_bins <= BESST_REPORT_MAX_ISIZE_BINS,
                  "dev_library_report: isize_bins must lie in 1 .. 2^20");
    const int64_t words = besst_dev_library_report_words(a->n_refs, a->isize_bins);
    BESST_REQUIRE(a->out_words >= words, "dev_library_report: the result buffer is too short");
    BESST_REQUIRE(a->n_records == 0 || (a->tid && a->mtid && a->pos && a->mpos && a->tlen && a->flag && a->mapq && a->qlen),
                  "dev_library_report: null column");
    hipStream_t s = static_cast<hipStream_t>(stream);
    BESST_HIP_TRY(hipMemsetAsync(out, 0, (size_t)words * 8, s));
    return launch_library_report(s, *a, reinterpret_cast<unsigned long long*>(out));
}

int besst_ctx_library_report(besst_ctx* c, int64_t isize_bins, uint64_t* out_host, int64_t out_words) {
    BESST_REQUIRE(c && out_host, "library_report: null pointer");
    BESST_REQUIRE(isize_bins >= 1 && isize_bins <= BESST_REPORT_MAX_ISIZE_BINS, "library_report: isize_bins must lie in 1 .. 2^20");
    const int64_t words = besst_dev_library_report_words(c->n_contigs, isize_bins);
    BESST_REQUIRE(words > 0 && out_words >= words, "library_report: the result buffer is too short");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = c->aux.ensure((size_t)words * 8))) return rc;
    besst_report_args a{};
    a.tid = c->tid.p; a.mtid = c->mtid.p; a.pos = c->pos.p; a.mpos = c->mpos.p; a.tlen = c->tlen.p;
    a.flag = c->flag.p; a.mapq = c->mapq.p; a.qlen = c->qlen.p;
    a.tid_bits = nullptr;
    a.n_records = c->n_records;
    a.n_refs = c->n_contigs;
    a.isize_bins = isize_bins;
    a.out_words = words;
    uint64_t* d_out = reinterpret_cast<uint64_t*>(c->aux.p);
    if ((rc = besst_dev_library_report(c->stream, &a, d_out))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(out_host, d_out, (size_t)words * 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int besst_ctx_metrics_sample(besst_ctx* c, const uint8_t* top_mask, int32_t orientation, int32_t min_mapq,
                             double read_len, int32_t want_isize, int32_t* isize_out, int32_t* contam_out,
                             besst_metrics_counts* counts) {
    BESST_REQUIRE(c && top_mask && contam_out && counts, "metrics_sample: null pointer");
    BESST_REQUIRE(!want_isize || isize_out, "metrics_sample: isize_out is null");
    BESST_REQUIRE(orientation == 0 || orientation == 1, "metrics_sample: orientation must be 0 or 1");
    if (c->n_contigs <= 0) {
        set_error("metrics_sample: set_contigs must be called first (defines the reference count)");
        return BESST_ERR_STATE;
    }
    int rc = use_device(c);
    if (rc) return rc;
    constexpr int64_t kCap = 1000000;
    constexpr int64_t kChunk = 16 << 20;      // (most libraries fill their samples within it: one launch)
    if ((rc = c->top_mask.ensure((size_t)c->n_contigs))) return rc;
    if ((rc = c->sample_a.ensure((size_t)kCap))) return rc;
    if ((rc = c->sample_b.ensure((size_t)kCap))) return rc;
    // Chunks: the reference stops each scan at its 1,000,000th qualifying record (libmetrics.py:83,302), the host learns the
    // counts between chunks.  The first chunk is kChunk records; each later one is sized from the rate seen so far so that
    // it should finish the scan (x 1.25, at most kChunkMax): a launch + a round trip to the host per 4 M records was most of
    // the pass's time when the samples fill late (60 M records: 15 chunks, 1.1 ms for 0.18 ms worth of bytes).
    constexpr int64_t kChunkMax = (int64_t)256 << 20;
    const int64_t ws_records = c->n_records < kChunkMax ? (c->n_records > kChunk ? c->n_records : kChunk) : kChunkMax;
    if ((rc = c->aux.ensure(metrics_workspace_bytes(ws_records) + 64))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(c->top_mask.p, top_mask, (size_t)c->n_contigs, hipMemcpyHostToDevice, c->stream));
    int64_t* state = reinterpret_cast<int64_t*>(c->aux.p);
    char* ws = c->aux.p + 64;
    BESST_HIP_TRY(hipMemsetAsync(state, 0, 64, c->stream));
    MetricsArgs a;
    a.tid = c->tid.p; a.mtid = c->mtid.p; a.tlen = c->tlen.p; a.flag = c->flag.p; a.mapq = c->mapq.p;
    a.top_mask = c->top_mask.p;
    a.n = c->n_records;
    a.n_contigs = (int32_t)c->n_contigs;
    a.rf = orientation;
    a.min_mapq = min_mapq;
    a.read_len = read_len;
    int64_t host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t next = kChunk;
    for (int64_t start = 0; start < c->n_records;) {
        const int64_t cnt = c->n_records - start < next ? c->n_records - start : next;
        rc = launch_metrics(c->stream, a, start, cnt, want_isize ? c->sample_a.p : nullptr, c->sample_b.p, state, ws,
                            c->aux.cap - 64);
        if (rc) return rc;
        BESST_HIP_TRY(hipMemcpyAsync(host, state, 48, hipMemcpyDeviceToHost, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
        start += cnt;
        // the reference stops each scan once its 1,000,000-sample cut-off is reached (libmetrics.py:83,302)
        if ((!want_isize || host[0] >= kCap) && host[1] >= kCap) break;
        // records still to scan at the rate of the slower of the two counts (none seen yet: as many as allowed)
        const int64_t slow = (want_isize && host[0] < host[1]) ? host[0] : host[1];
        double need = slow > 0 ? (double)(kCap - slow) * (double)start / (double)slow * 1.25 : (double)kChunkMax;
        if (need > (double)kChunkMax) need = (double)kChunkMax;
        next = ((int64_t)need + kChunk - 1) / kChunk * kChunk;   // (a multiple of 4: launch_metrics wants aligned starts)
        if (next < kChunk) next = kChunk;
    }
    counts->n_isize = want_isize ? (host[0] < kCap ? host[0] : kCap) : 0;
    counts->sample_counter = host[1] < kCap ? host[1] : kCap;
    counts->counter_total = host[3];
    counts->n_contam = host[4];
    counts->records_scanned = host[5];
    if (counts->n_isize)
        BESST_HIP_TRY(hipMemcpyAsync(isize_out, c->sample_a.p, (size_t)counts->n_isize * 4, hipMemcpyDeviceToHost, c->stream));
    if (counts->n_contam)
        BESST_HIP_TRY(hipMemcpyAsync(contam_out, c->sample_b.p, (size_t)counts->n_contam * 4, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int besst_ctx_value_histogram(besst_ctx* c, const int32_t* values, int64_t n, int64_t n_bins, int64_t* hist_out,
                              int64_t* overflow) {
    BESST_REQUIRE(c && hist_out && overflow, "value_histogram: null pointer");
    BESST_REQUIRE(n >= 0 && n_bins > 0 && n_bins < ((int64_t)1 << 31), "value_histogram: size out of range");
    BESST_REQUIRE(n == 0 || values, "value_histogram: null values");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = c->sample_a.ensure((size_t)(n > 0 ? n : 1)))) return rc;
    if ((rc = c->aux.ensure((size_t)(n_bins + 1) * 8))) return rc;
    auto* hist = reinterpret_cast<unsigned long long*>(c->aux.p);
    BESST_HIP_TRY(hipMemsetAsync(hist, 0, (size_t)(n_bins + 1) * 8, c->stream));
    if (n) BESST_HIP_TRY(hipMemcpyAsync(c->sample_a.p, values, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_value_histogram(c->stream, c->sample_a.p, n, n_bins, hist, hist + n_bins))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(hist_out, hist, (size_t)n_bins * 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(overflow, hist + n_bins, 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

int besst_dev_gap_condition_table(void* stream, double mean, double sigma, double read_len, double contig_len,
                                  int32_t d_lower, int32_t n, double* out) {
    BESST_REQUIRE(n >= 0 && (n == 0 || out) && sigma > 0.0, "gap_condition_table: bad argument");
    return launch_gap_table(static_cast<hipStream_t>(stream), mean, sigma, read_len, contig_len, d_lower, n, out);
}

int besst_ctx_gap_condition_table(besst_ctx* c, double mean, double sigma, double read_len, double contig_len,
                                  int32_t d_lower, int32_t n, double* h_out) {
    BESST_REQUIRE(c && n >= 0 && (n == 0 || h_out) && sigma > 0.0, "gap_condition_table: bad argument");
    if (n == 0) return BESST_OK;
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = c->aux.ensure((size_t)n * sizeof(double)))) return rc;
    auto* d_out = reinterpret_cast<double*>(c->aux.p);
    if ((rc = launch_gap_table(c->stream, mean, sigma, read_len, contig_len, d_lower, n, d_out))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

namespace {
// besst_ctx_score_edges / besst_ctx_score_edges_lognormal: upload the edge list, lay the scratch out, run, download.
int ctx_score_impl(besst_ctx* c, int64_t n_edges, const uint32_t* row, const uint8_t* swap, const int32_t* len1,
                   const int32_t* len2, double mean, double sigma, double read_len, const LogNormalArgs* ln, double* gap,
                   double* sd0, int32_t* ks_h, uint8_t* flags) {
    int rc;
    // scratch offsets for edges too large for the LDS sort
    std::vector<uint32_t> h_n((size_t)c->n_rows);
    BESST_HIP_TRY(hipMemcpyAsync(h_n.data(), c->row_n.p, (size_t)c->n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> big_off((size_t)n_edges, 0ull);
    unsigned long long big_total = 0;
    for (int64_t e = 0; e < n_edges; ++e) {
        BESST_REQUIRE((int64_t)row[e] < c->n_rows, "score_edges: row index out of range");
        const uint32_t n = h_n[row[e]];
        BESST_REQUIRE(n >= 1, "score_edges: empty row");
        unsigned long long np = 1;
        while (np < n) np <<= 1;
        if (np > 8192) { big_off[(size_t)e] = big_total; big_total += 2 * np; }
    }
    const size_t m = (size_t)n_edges;
    const size_t in_bytes = align_up(m * 4, 256) + align_up(m, 256) + 2 * align_up(m * 4, 256);
    const size_t out_bytes = 2 * align_up(m * 8, 256) + align_up(m * 4, 256) + align_up(m, 256);
    const size_t ws_bytes = align_up(m * 8, 256) + align_up((size_t)big_total * 4 + 4, 256);
    if ((rc = c->aux.ensure(in_bytes + out_bytes + ws_bytes))) return rc;
    char* p = c->aux.p;
    auto take = [&p](size_t bytes) { char* q = p; p += align_up(bytes, 256); return q; };
    auto* d_row = reinterpret_cast<uint32_t*>(take(m * 4));
    auto* d_swap = reinterpret_cast<uint8_t*>(take(m));
    auto* d_len1 = reinterpret_cast<int32_t*>(take(m * 4));
    auto* d_len2 = reinterpret_cast<int32_t*>(take(m * 4));
    auto* d_gap = reinterpret_cast<double*>(take(m * 8));
    auto* d_sd0 = reinterpret_cast<double*>(take(m * 8));
    auto* d_ks = reinterpret_cast<int32_t*>(take(m * 4));
    auto* d_flags = reinterpret_cast<uint8_t*>(take(m));
    char* d_ws = p;
    BESST_HIP_TRY(hipMemcpyAsync(d_row, row, m * 4, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(d_swap, swap, m, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(d_len1, len1, m * 4, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(d_len2, len2, m * 4, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(d_ws, big_off.data(), m * 8, hipMemcpyHostToDevice, c->stream));
    ScoreArgs a;
    a.row = d_row; a.swap = d_swap; a.len1 = d_len1; a.len2 = d_len2;
    a.row_n = c->row_n.p; a.row_sum = c->row_sum.p; a.row_offset = c->row_offset.p;
    a.obs_lo = c->obs_lo.p; a.obs_hi = c->obs_hi.p;
    a.mean = mean; a.sigma = sigma; a.read_len = read_len;
    a.n_edges = n_edges;
    if (ln) rc = launch_score_lognormal(c->stream, a, *ln, d_gap, d_sd0, d_ks, d_flags, d_ws, ws_bytes);
    else rc = launch_score(c->stream, a, d_gap, d_sd0, d_ks, d_flags, d_ws, ws_bytes);
    if (rc) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(gap, d_gap, m * 8, hipMemcpyDeviceToHost, c->stream));
    if (sd0) BESST_HIP_TRY(hipMemcpyAsync(sd0, d_sd0, m * 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(ks_h, d_ks, m * 4, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(flags, d_flags, m, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}
}  // namespace

int besst_ctx_score_edges(besst_ctx* c, int64_t n_edges, const uint32_t* row, const uint8_t* swap, const int32_t* len1,
                          const int32_t* len2, double mean, double sigma, double read_len, double* gap, double* sd0,
                          int32_t* ks_h, uint8_t* flags) {
    BESST_NEED_BUILT(c);
    BESST_REQUIRE(n_edges >= 0, "score_edges: negative edge count");
    if (n_edges == 0) return BESST_OK;
    BESST_REQUIRE(row && swap && len1 && len2 && gap && sd0 && ks_h && flags, "score_edges: null pointer");
    BESST_REQUIRE(sigma > 0.0, "score_edges: sigma must be positive");
    int rc = use_device(c);
    if (rc) return rc;
    return ctx_score_impl(c, n_edges, row, swap, len1, len2, mean, sigma, read_len, nullptr, gap, sd0, ks_h, flags);
}

int besst_ctx_score_edges_lognormal(besst_ctx* c, int64_t n_edges, const uint32_t* row, const uint8_t* swap,
                                    const int32_t* len1, const int32_t* len2, double mean, double sigma, double read_len,
                                    double ln_mu, double ln_sigma, int64_t x_max, int32_t max_gap, double* gap,
                                    int32_t* ks_h, uint8_t* flags) {
    BESST_NEED_BUILT(c);
    BESST_REQUIRE(n_edges >= 0, "score_edges_lognormal: negative edge count");
    if (n_edges == 0) return BESST_OK;
    BESST_REQUIRE(row && swap && len1 && len2 && gap && ks_h && flags, "score_edges_lognormal: null pointer");
    BESST_REQUIRE(sigma > 0.0 && ln_sigma > 0.0, "score_edges_lognormal: sigma must be positive");
    BESST_REQUIRE(x_max >= 1 && x_max < ((int64_t)1 << 31) && max_gap >= 0, "score_edges_lognormal: parameters out of range");
    int rc = use_device(c);
    if (rc) return rc;
    // [ F0 | F1 | G0 | G1 ]: prefix tables of x_max + 1 entries, tail tables of lognormal_tail_entries
    const size_t ne = (size_t)lognormal_tail_entries(ln_mu, x_max);
    double* const F0 = c->ln_tables.p;
    if (!(F0 && c->ln_mu == ln_mu && c->ln_sigma == ln_sigma && c->ln_x_max == x_max)) {
        c->ln_x_max = 0;
        if ((rc = c->ln_tables.ensure(2 * (size_t)(x_max + 1) + 2 * ne))) return rc;
        double* const T = c->ln_tables.p;
        const size_t wsb = lognormal_tables_workspace_bytes(x_max);
        if ((rc = c->aux.ensure(wsb))) return rc;
        if ((rc = launch_lognormal_tables(c->stream, ln_mu, ln_sigma, x_max, T, T + (x_max + 1), c->aux.p, wsb))) return rc;
        if ((rc = launch_lognormal_tails(c->stream, ln_mu, ln_sigma, x_max, T + 2 * (x_max + 1), T + 2 * (x_max + 1) + ne,
                                         c->aux.p, wsb)))
            return rc;
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));          // aux is laid out anew below
        c->ln_mu = ln_mu; c->ln_sigma = ln_sigma; c->ln_x_max = x_max;
    }
    const double* const T = c->ln_tables.p;
    LogNormalArgs ln{ln_mu, ln_sigma, x_max, T, T + (x_max + 1), max_gap, T + 2 * (x_max + 1), T + 2 * (x_max + 1) + ne};
    return ctx_score_impl(c, n_edges, row, swap, len1, len2, mean, sigma, read_len, &ln, gap, nullptr, ks_h, flags);
}

int besst_ctx_conditional_stddevs(besst_ctx* c, const double* density, int64_t max_isize, const int32_t* steps,
                                  int32_t n_steps, double* h_out) {
    BESST_REQUIRE(c, "conditional_stddevs: null context");
    BESST_REQUIRE(n_steps >= 0 && max_isize >= 0, "conditional_stddevs: negative size");
    if (n_steps == 0) return BESST_OK;
    BESST_REQUIRE(density && steps && h_out, "conditional_stddevs: null pointer");
    int rc = use_device(c);
    if (rc) return rc;
    const size_t fb = align_up((size_t)(max_isize + 1) * 8, 256), sb = align_up((size_t)n_steps * 4, 256);
    if ((rc = c->aux.ensure(fb + sb + align_up((size_t)n_steps * 8, 256)))) return rc;
    auto* d_f = reinterpret_cast<double*>(c->aux.p);
    auto* d_steps = reinterpret_cast<int32_t*>(c->aux.p + fb);
    auto* d_out = reinterpret_cast<double*>(c->aux.p + fb + sb);
    BESST_HIP_TRY(hipMemcpyAsync(d_f, density, (size_t)(max_isize + 1) * 8, hipMemcpyHostToDevice, c->stream));
    BESST_HIP_TRY(hipMemcpyAsync(d_steps, steps, (size_t)n_steps * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_conditional_stddevs(c->stream, d_f, max_isize, d_steps, n_steps, d_out))) return rc;
    BESST_HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)n_steps * 8, hipMemcpyDeviceToHost, c->stream));
    BESST_HIP_TRY(hipStreamSynchronize(c->stream));
    return BESST_OK;
}

}  // extern "C"
