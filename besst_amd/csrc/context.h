// The HBM-owning context behind the C ABI's besst_ctx handle, for the two files that reach into it: api.hip and ingest.hip.
#pragma once

#include <type_traits>

#include "common.h"

namespace besst {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    int ensure(size_t n) {
        if (n <= cap) return BESST_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 8 + 64;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
            return BESST_ERR_NOMEM;
        }
        cap = want;
        return BESST_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace besst

struct besst_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // contig table
    int64_t n_contigs = 0;
    int32_t node_bits = 1;
    uint64_t key_base = 0;
    int32_t key_bits = 3;
    besst::DevBuf<besst::ContigRow> table;
    besst::DevBuf<int64_t> aligned;
    // library
    bool have_lib = false;
    besst_lib_params lib{};
    // resident records
    int64_t n_records = 0;
    besst::DevBuf<int32_t> tid, mtid, pos, mpos, tlen;
    besst::DevBuf<uint16_t> flag, qlen;
    besst::DevBuf<uint8_t> mapq;
    besst::DevBuf<uint8_t> mate_bits;       // one bit per record: tid != mtid (ClassifyArgs::mate_bits), valid for the first bits_upto records
    int64_t bits_upto = 0;
    besst::DevBuf<uint8_t> tid_bits;        // one bit per record: tid differs from the record before (ClassifyArgs::tid_bits), valid for the first tid_bits_upto records
    int64_t tid_bits_upto = 0;
    // the candidate side stream of the resident records (besst_cand_stream; ClassifyArgs::cs_*), made for cs.n_refs
    // references and valid for the first cs_upto records: extended at a build, from the block that held record cs_upto,
    // for what was pushed since; made anew when a buffer has to grow or the contig count is another
    besst::DevBuf<uint8_t> cs_set, cs_entries;
    besst::DevBuf<uint32_t> cs_off;
    besst_cand_stream cs{};
    int64_t cs_upto = 0;
    int64_t cs_cap_entries = 0;             // entries a column of cs_entries holds (the columns' stride)
    // (a device ingest - ingest.hip - writes the planes and the stream while it decodes and moves the three watermarks
    // itself; a build then finds nothing to make)
    int64_t maker_launches = 0;             // launches of the planes' and the stream's makers by besst_ctx_build_graph
    // tuple stream + edge table
    besst::DevBuf<uint64_t> keys, payload, row_key;
    besst::DevBuf<uint32_t> row_mask, row_n, row_first, row_offset;
    besst::DevBuf<int64_t> row_sum, row_sum_sq;
    besst::DevBuf<int32_t> obs_lo, obs_hi;
    besst::DevBuf<int32_t> obs_sum;         // besst_ctx_fetch_observation_sums: obs_lo + obs_hi, made and copied on side_stream
    hipStream_t side_stream = nullptr;
    besst::DevBuf<char> ws;
    besst::DevBuf<char> small;      // counters + carry + n_out + n_rows
    bool built = false;
    int64_t n_rows = 0, n_tuples = 0;
    // misc scratch for metrics / scoring
    besst::DevBuf<uint8_t> top_mask;
    besst::DevBuf<int32_t> sample_a, sample_b;
    besst::DevBuf<char> aux;
    // prefix tables of the log-normal pmf (besst_ctx_score_edges_lognormal), kept while (mu, sigma, x_max) stay the same
    besst::DevBuf<double> ln_tables;
    double ln_mu = 0.0, ln_sigma = 0.0;
    int64_t ln_x_max = 0;
    // SAM text ingest (sam.hip): the reference table of besst_ctx_set_sam_references (slots, the names end to end, their
    // offsets), the tile scratch and line rows of a chunk, the head arrays of the first records
    besst::DevBuf<uint32_t> sam_slots, sam_rows;
    besst::DevBuf<uint8_t> sam_pool;
    besst::DevBuf<int64_t> sam_off;
    besst::DevBuf<char> sam_ws, sam_head;
    uint32_t sam_cap = 0;
    int64_t sam_refs = 0;
    // besst_ctx_sam_expect_text: the record text announced for the file being pushed, what of it has come, its records
    int64_t sam_expect_bytes = 0, sam_seen_bytes = 0, sam_file_records = 0;
    bool sam_timing = false;                // besst_ctx_sam_pass_times: events around the four passes of every push
    double sam_ms[4] = {0.0, 0.0, 0.0, 0.0};
};

namespace besst {

struct SmallBlock {
    besst_counters counters;
    int32_t carry[2];
    uint32_t n_out;
    uint32_t n_rows;
};

// joins the threads that free an ingest's device scratch (ingest.hip): before a context goes
void ingest_join_background();

inline int use_device(besst_ctx* c) {
    BESST_HIP_TRY(hipSetDevice(c->device));
    return BESST_OK;
}

// Reserve room for `total` records in every column, carrying the first `have` over (one reallocation + device copy instead
// of a chain of them).
inline int reserve_records(besst_ctx* c, int64_t have, int64_t total) {
    auto grow = [&](auto& buf) -> int {
        using T = typename std::remove_reference<decltype(*buf.p)>::type;
        if ((size_t)total <= buf.cap) return BESST_OK;
        DevBuf<T> bigger;
        int rc = bigger.ensure((size_t)total);
        if (rc) return rc;
        if (have) BESST_HIP_TRY(hipMemcpyAsync(bigger.p, buf.p, (size_t)have * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        BESST_HIP_TRY(hipStreamSynchronize(c->stream));
        buf.release();
        buf = bigger;
        return BESST_OK;
    };
    int rc;
    if ((rc = grow(c->tid)) || (rc = grow(c->mtid)) || (rc = grow(c->pos)) || (rc = grow(c->mpos)) || (rc = grow(c->tlen)) ||
        (rc = grow(c->flag)) || (rc = grow(c->mapq)) || (rc = grow(c->qlen)))
        return rc;
    return BESST_OK;
}

}  // namespace besst
