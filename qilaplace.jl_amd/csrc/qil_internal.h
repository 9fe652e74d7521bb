// Internal declarations shared by the libqilhip.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_complex.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <condition_variable>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "qilaplace_hip.h"
#include "qilaplace_hip_testing.h"

#include <atomic>

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE (a `static bool` granted it on the first GPU only,
// and a context on a second GPU of the same process then failed its launch).  One of these per kernel: the bytes granted so
// far on each device; concurrent callers may both set the attribute, which is harmless.
struct qil_lds_grant {
    static constexpr int kDevices = 64;
    std::atomic<size_t> bytes[kDevices] = {};
    hipError_t ensure(int device, const void* fn, size_t want) {
        const int d = device >= 0 && device < kDevices ? device : -1;
        if (d >= 0 && want <= bytes[d].load(std::memory_order_acquire)) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
        if (e == hipSuccess && d >= 0) {
            size_t cur = bytes[d].load(std::memory_order_relaxed);
            while (cur < want && !bytes[d].compare_exchange_weak(cur, want, std::memory_order_release)) {}
        }
        return e;
    }
};

// ---------------------------------------------------------------- errors
void qil_set_error(const char* fmt, ...);
int qil_fail(int code, const char* fmt, ...);

#define QIL_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return qil_fail(_e == hipErrorOutOfMemory ? QIL_ENOMEM : QIL_EHIP,             \
                            "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),         \
                            __FILE__, __LINE__);                                           \
    } while (0)

#define QIL_TRY(expr)                 \
    do {                              \
        int _s = (expr);              \
        if (_s != QIL_OK) return _s;  \
    } while (0)

#define QIL_REQUIRE(cond, code, ...)                       \
    do {                                                   \
        if (!(cond)) return qil_fail((code), __VA_ARGS__); \
    } while (0)

// ---------------------------------------------------------------- context
struct qil_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // caching pool: exact-size free lists (apply outputs recur with identical sizes)
    std::multimap<size_t, void*> free_blocks;
    struct live_block {
        size_t bytes;
        uint64_t serial;   // allocation order (error-path reclamation, see qil_call_scope)
        bool owned;        // attached to a chain handle: outlives the call that allocated it
    };
    std::map<void*, live_block> live_blocks;
    uint64_t alloc_serial = 0;
    int64_t fail_alloc_countdown = -1;   // fault injection (qil_context_fail_alloc_after); < 0 = off
    size_t bytes_in_use = 0, bytes_cached = 0;
    // pinned staging for small descriptor / bit uploads
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    struct qil_lockstep* lockstep = nullptr;   // set while this context is a slot of a running lock-step batch (qil_launch.h)
    int ls_slot = 0;              // ... and which one
    hipEvent_t sync_event = nullptr;   // qil_stream_sync inside a lock-step batch
    uint64_t progress_key = 0;    // where the chain driven through this context is (qil_progress)
    int cholqr_skip = 0;          // Cholesky QR attempts to skip after a refusal (qr_impl)
    struct qil_qr_report* qr_report = nullptr;   // where qr_impl, cholqr2 and qr_reorthogonalise say what they did; null outside qil_qr_host
    // small device -> host read-backs without a copy command or a stream synchronisation (qil_read_back): kRbSlots slots of
    // kRbSlotBytes in pinned, device-visible memory + a ticket word a kernel writes behind the data; the host polls the word
    static constexpr int kRbSlots = 4;
    static constexpr size_t kRbSlotBytes = 8192;
    void* rb_host = nullptr;
    uint64_t rb_ticket = 0, rb_done = 0;                          // posted / seen complete
    bool dbg_times = false;       // QIL_BATCH_DEBUG: where a chain's host thread spends its time
    double dbg_rb_us = 0, dbg_ring_us = 0, dbg_alloc_us = 0;
    long long dbg_rb_n = 0, dbg_alloc_n = 0, dbg_alloc_miss = 0;
    // small host -> device uploads of a chain (permutations, scale vectors) without a copy command or an event: filled in a
    // pinned slot, moved by a (combinable) copy kernel; a slot is reused once a read-back posted after its consumers has
    // completed (qil_stage_*)
    static constexpr int kStSlots = 16;
    static constexpr size_t kStSlotBytes = 32768;
    void* st_host = nullptr;
    void* st_dev = nullptr;
    uint64_t st_born[kStSlots] = {};
    bool st_used[kStSlots] = {};
    int st_next = 0;
    void* dev_scratch = nullptr;  // per-call device workspace (stream-ordered reuse)
    size_t dev_scratch_bytes = 0;
    // ring of small host(pinned)/device descriptor slots for grouped launches: a slot is reused
    // only after the event recorded behind its last consumer has completed
    static constexpr int kDescSlots = 8;
    static constexpr size_t kDescSlotBytes = 1 << 16;
    void* desc_host = nullptr;
    void* desc_dev = nullptr;
    hipEvent_t desc_event[kDescSlots] = {};
    bool desc_used[kDescSlots] = {};
    int desc_next = 0;
    // timers
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    std::vector<hipEvent_t> event_pool;
    int num_cus = 256;
    // live chain handles: orphaned (ctx = nullptr, site pointers dropped) when the context is destroyed first,
    // so a handle released after its context touches nothing
    std::set<struct qil_chain*> chains;
    // communicators created on this context (qil_comm.hip): torn down with it, their handles stay valid and empty
    std::set<struct qil_comm*> comms;
    // Batch entry points (qil_run_batch): independent chains run concurrently on this context's own stream (calling
    // thread) and on worker contexts (own stream and pool, one host thread each), one batch at a time.  For the duration of
    // a batch the home context's cached blocks are LENT: every participant misses in its own cache first, then takes from
    // `lend_blocks` (all work enqueued on them is ordered before the batch by an event), then allocates; at the end the
    // remaining lent blocks return to the home cache and the workers keep theirs, so steady-state batches allocate nothing and
    // take (almost) nothing from the lender.
    std::vector<qil_context*> workers;
    std::mutex batch_mutex;
    qil_context* parent = nullptr;                   // worker -> home
    bool lending = false;                            // home: a batch is running
    std::multimap<size_t, void*> lend_blocks;        // guarded by pool_mutex
    size_t lend_cached = 0;                          // bytes in lend_blocks (guarded by pool_mutex)
    std::mutex pool_mutex;
};

// The stream for anything that is NOT a qil_klaunch: inside a lock-step batch the chain first waits until the launcher has
// issued everything it has queued (stream order), otherwise this is ctx->stream.
void qil_lockstep_drain(qil_context* ctx);
inline hipStream_t qil_stream(qil_context* ctx) {
    if (ctx->lockstep) qil_lockstep_drain(ctx);
    return ctx->stream;
}
// hipStreamSynchronize for chain code: inside a lock-step batch the slots share one stream that the launcher keeps feeding, so
// the chain waits for an event recorded behind ITS last operation instead of for the whole stream to run dry
hipError_t qil_stream_sync(qil_context* ctx);
hipError_t qil_event_sync(qil_context* ctx, hipEvent_t ev);    // hipEventSynchronize that tells the batch's launcher the chain is parked
int qil_ctx_activate(qil_context* ctx);  // hipSetDevice
int qil_ctx_alloc(qil_context* ctx, size_t bytes, void** out);
int qil_ctx_free(qil_context* ctx, void* p);
int qil_ctx_pinned(qil_context* ctx, size_t bytes, void** out);       // grows, stream-synchronising
int qil_ctx_dev_scratch(qil_context* ctx, size_t bytes, void** out);  // grows
// A host table on the device for one grouped launch -- what every grouped launch goes through.  upload() takes the descriptor
// ring where the table fits a slot, a pool block otherwise (filled from the pageable source and stream-synchronised); a second
// span, if given, lands right behind the first (at dev + bytes).  release() hands the slot back committed behind whatever was
// enqueued, or the block to the pool, which recycles in stream order; call it after the last consumer launch.  The destructor
// releases what an early return left, so a failing launch can never strand a slot without its event.
struct qil_dev_table {
    qil_context* ctx;
    void* dev = nullptr;
    void* block = nullptr;
    int slot = -1;
    explicit qil_dev_table(qil_context* c) : ctx(c) {}
    ~qil_dev_table() { release(); }
    qil_dev_table(const qil_dev_table&) = delete;
    qil_dev_table& operator=(const qil_dev_table&) = delete;
    int upload(const void* src, size_t bytes, const void* src2 = nullptr, size_t bytes2 = 0);
    int release();
    template <class T>
    const T* as(size_t byte_offset = 0) const {
        return reinterpret_cast<const T*>(static_cast<const char*>(dev) + byte_offset);
    }
};
// The pool temporaries of one call that live outside a handle.  alloc() takes a block from the context pool, own() takes in one
// that a callee returned (svd_trunc_dev's factors); free() returns one early, so the peak is what the algorithm needs; give() hands
// one to a handle (qil_chain_adopt, qil_chain_set_site) or to the caller.  The destructor frees what is left, on every return path.
// A block is listed at most once and leaves the list when it is freed or given, so none is freed twice: a second qil_ctx_free of
// an address puts an error behind a successful call (or, once the pool has handed the address out again, frees a stranger's
// block).  Declare it after the call's qil_call_scope: a failed call then frees these first and the scope reclaims the rest.
struct qil_scratch {
    qil_context* ctx;
    std::vector<void*> blocks;
    explicit qil_scratch(qil_context* c) : ctx(c) {}
    ~qil_scratch() {
        for (void* p : blocks) qil_ctx_free(ctx, p);
    }
    qil_scratch(const qil_scratch&) = delete;
    qil_scratch& operator=(const qil_scratch&) = delete;
    int alloc(size_t bytes, void** out) {
        const int s = qil_ctx_alloc(ctx, bytes, out);
        if (s == QIL_OK) blocks.push_back(*out);
        return s;
    }
    void* own(void* p) {
        blocks.push_back(p);
        return p;
    }
    void* give(void* p) {                      // the latest blocks leave first: search from the back
        for (size_t t = blocks.size(); t-- > 0;)
            if (blocks[t] == p) {
                blocks.erase(blocks.begin() + (long)t);
                return p;
            }
        return nullptr;                        // not ours (any more): nothing to hand over, nothing to free
    }
    void free(void* p) {
        if (give(p)) qil_ctx_free(ctx, p);
    }
};
int qil_ctx_event(qil_context* ctx, hipEvent_t* e);            // from the context's event pool
void qil_ctx_event_release(qil_context* ctx, hipEvent_t e);
// `bytes` (a multiple of 4, 4-byte aligned source) of device memory to the host, ordered after everything this context has
// launched: qil_read_back = post + wait; posted read-backs complete in order, at most kRbSlots - 1 may be outstanding.
// Larger blocks than a slot take the copy-command + stream-synchronisation route.
int qil_apply_shared_state(const qil_mpo* W, const qil_mps* psi, qil_mps** out);   // (qil_apply.hip) psi may live in another context of the device
int qil_check_apply_operands(const qil_mpo* W, const qil_mps* psi);   // (qil_apply.hip) the operand checks of qil_apply
int qil_lockstep_park(qil_context* ctx, const unsigned long long* word, unsigned long long ticket);   // (qil_context.hip)
int qil_read_back_post(qil_context* ctx, const void* dev_src, size_t bytes, uint64_t* ticket);
int qil_read_back_wait(qil_context* ctx, uint64_t ticket, void* host_dst, size_t bytes);
int qil_read_back(qil_context* ctx, void* host_dst, const void* dev_src, size_t bytes);
// acquire a slot (host = pinned side to fill, dev = what the kernels read), push = launch the copy, commit = the consumers
// have been launched
int qil_stage_acquire(qil_context* ctx, size_t bytes, void** host, void** dev, int* slot);
int qil_stage_push(qil_context* ctx, int slot, size_t bytes);
void qil_stage_commit(qil_context* ctx, int slot);
int qil_ctx_prof_begin(qil_context* ctx);
int qil_ctx_prof_end(qil_context* ctx);

// Batches of independent chains.  A chain of truncations is a latency chain of small dependent kernels that occupies a
// few percent of the chip; `fn` is run for every chain of the batch concurrently: chain j is handed (its pool blocks
// change owner, nothing is copied) to worker context j % nw of the chains' common home context, one host thread per worker
// drives it on that worker's stream, and the chains return to the home context before the call does.  The work of
// each chain is exactly what fn(chain) does alone.  All chains must belong to the same context; nw = min(nb,
// QIL_BATCH_WORKERS (default 8)).  Returns the first failing chain's status.
int qil_run_batch(struct qil_chain* const* items, int64_t nb, const std::function<int(struct qil_chain*)>& fn);
// The same for work that CREATES chains from read-only operands of the home context: fn(j, work) runs item j with `work`
// as its working context (stream + pool; operands may be shared between items and stay where they are); every chain
// bound to a worker when the batch ends -- moved there by place(j, slot) beforehand or created by fn -- returns to home.
int qil_run_batch_on(qil_context* home, int64_t nb, const std::function<void(int64_t, qil_context*)>& place,
                     const std::function<int(int64_t, qil_context*)>& fn);
void qil_comm_orphan(struct qil_comm* cm);   // (qil_comm.hip) the context of a communicator is going away
// hand a live pool block of `from` to `to` (bookkeeping only; the caller orders the streams)
void qil_ctx_transfer(qil_context* from, qil_context* to, void* p);
// hand a whole chain (its site blocks and its registration) to another context of the same device
void qil_chain_rebind(struct qil_chain* c, qil_context* to);
// device copy of psi owned by ctx (made on ctx's stream)
int qil_mps_clone_to(qil_context* ctx, const struct qil_mps* psi, struct qil_mps** out);

// ---------------------------------------------------------------- containers
static inline size_t qil_elem_size(int dtype) { return dtype == QIL_C64 ? 16 : 8; }

struct qil_chain {
    qil_context* ctx = nullptr;
    int dtype = QIL_F64;
    int paired = 0;
    int phys_rank = 1;               // 1 = MPS (A[a,s,b]), 2 = MPO (W[a,si,so,b])
    std::vector<int64_t> dims;       // n+1 bond dims incl. the two dim-1 edges
    std::vector<int64_t> site_ids;   // n labels
    std::vector<void*> site;         // device pointers, one allocation per site
    double amplitude = 1.0;
    qil_chain() = default;
    qil_chain(const qil_chain&) = delete;
    qil_chain& operator=(const qil_chain&) = delete;
    ~qil_chain() {
        if (ctx) ctx->chains.erase(this);
    }
    int64_t n() const { return (int64_t)site.size(); }
    int64_t site_elems(int64_t i) const {
        return dims[i] * (phys_rank == 1 ? 2 : 4) * dims[i + 1];
    }
    size_t site_bytes(int64_t i) const { return (size_t)site_elems(i) * qil_elem_size(dtype); }
};
struct qil_mps : qil_chain {};
struct qil_mpo : qil_chain {};

int qil_chain_alloc(qil_context* ctx, qil_chain* c, int64_t n, int dtype, int paired, int phys_rank,
                    const int64_t* bond_dims, const int64_t* site_ids);
int qil_chain_release(qil_chain* c);
// a bound MPS of n empty site slots with all bonds 1, for a result built site by site (qil_chain_adopt / qil_chain_set_site);
// site_ids = nullptr numbers the sites 1..n.  Allocates nothing on the device.
struct qil_mps* qil_mps_empty(qil_context* ctx, int64_t n, int dtype, int paired, const int64_t* site_ids, double amplitude);
// tie a handle to its context (registers it for orphaning on context destruction)
void qil_chain_bind(qil_chain* c, qil_context* ctx);
// replace site i's buffer (takes ownership of `p`), updating the bond dims
int qil_chain_set_site(qil_chain* c, int64_t i, void* p, int64_t dl, int64_t dr);
// attach a pool block to an EMPTY site slot of a chain under construction (ownership moves to the chain)
void qil_chain_adopt(qil_chain* c, int64_t i, void* p);
// Owns a result handle (qil_mps or qil_mpo) while the call that allocated it can still fail: the sites belong to the handle, not
// to the call scope, so every early return destroys it; release() hands it to the caller on success.
inline void qil_handle_destroy(qil_mps* p) { qil_mps_destroy(p); }
inline void qil_handle_destroy(qil_mpo* p) { qil_mpo_destroy(p); }
template <class H>
struct qil_result_guard {
    H* p = nullptr;
    explicit qil_result_guard(H* h) : p(h) {}
    ~qil_result_guard() {
        if (p) qil_handle_destroy(p);
    }
    qil_result_guard(const qil_result_guard&) = delete;
    qil_result_guard& operator=(const qil_result_guard&) = delete;
    qil_result_guard(qil_result_guard&& o) noexcept : p(o.release()) {}     // for a std::vector of guards
    H* release() {
        H* h = p;
        p = nullptr;
        return h;
    }
};

// Error-path reclamation.  Every C entry point opens one of these; temporaries come from the context pool and
// are released explicitly on the success path.  If the call FAILS (qil_fail ran on this thread while the scope
// was open), the destructor returns to the pool every block that was allocated during the call and is not
// owned by a chain handle -- so an early `return status` can never strand device memory.
unsigned qil_fail_count();
struct qil_call_scope {
    qil_context* ctx;
    uint64_t serial0;
    unsigned fails0;
    explicit qil_call_scope(qil_context* c);
    ~qil_call_scope();
    qil_call_scope(const qil_call_scope&) = delete;
    qil_call_scope& operator=(const qil_call_scope&) = delete;
};

// (qil_sample.hip) the trace-normalised right environments of qil_sample: R_n = [1], R_{i-1} = sum_s A_i[:, s, :] R_i A_i[:, s, :]^H
// scaled by 1 / Re tr, in one block of tmp (*Rall, bond b's chi_b x chi_b matrix at element roff[b]); the pass's own two
// temporaries come from tmp and go back before it returns.  log_norm2 (nullable, host) receives the sum of the log traces,
// log |psi|^2 without the amplitude.  QIL_EDOMAIN ("<verb>: the state has zero norm") for a state of norm 0.
int qil_dev_right_envs(const struct qil_mps* psi, qil_scratch& tmp, const char* verb, void** Rall, std::vector<long long>& roff,
                       double* log_norm2);

// ---------------------------------------------------------------- device linear algebra (qil_linalg.hip)
// All matrices column-major on the device, dtype QIL_F64/QIL_C64.
// C[m x n] = opA(A) * opB(B); op: 0 = N, 1 = T, 2 = H, 3 = conj (no transpose).  alpha = 1, beta = 0.
int qil_dev_gemm(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                 const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc);
// The same product for a SKINNY op(A) (m <= 48 rows against thousands of columns: the bit-sorted coefficient read-out):
// 32 x 64 / 48 x 64 output tiles with two K tiles in flight instead of 64 x 64 with one, so that a 30-row operand does not pay
// for 64 rows of matrix-core work and the long operand streams at more than one tile's latency allows.
int qil_dev_gemm_skinny(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                        const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc);
// Strided batch of the same product (grid y = batch): operand/result b lives at base + b * stride elements;
// optionally B of batch b is shifted by b_sel[b * b_sel_step] * b_sel_stride further elements.  A count above the grid's
// y limit goes out in pieces of 65535.
struct qil_gemm_batch {
    int64_t count = 1;
    int64_t a_bs = 0, b_bs = 0, c_bs = 0;
    const uint8_t* b_sel = nullptr;
    int64_t b_sel_step = 0, b_sel_stride = 0;
};
int qil_dev_gemm_batched(qil_context* ctx, int dtype, int opA, int opB, int64_t m, int64_t n, int64_t k,
                         const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                         const qil_gemm_batch* batch);
// A table of SMALL independent products in ONE launch (qil_sum.hip): C (m x n, ldc) = A (m x k, lda) * B (k x n, ldb), all of
// one dtype, one 16 x 16 f64-MFMA tile per wave, no LDS.  For steps that would otherwise
// cost one ~4 us dispatch per operand for a microsecond of work (the per-term products of qil_mps_sum_compress); tile_begin is
// filled in by the call.  qil_dev_gemm_grouped_fits: the table fits one descriptor slot (what qil_sum_compress_impl routes by).
struct qil_gemm_problem {
    const void* A;
    const void* B;
    void* C;
    int m, n, k;
    int lda, ldb, ldc;
    int tile_begin;
    int pad;
};
int qil_dev_gemm_grouped(qil_context* ctx, int dtype, std::vector<qil_gemm_problem>& probs);
bool qil_dev_gemm_grouped_fits(size_t nproblems);
// (qil_readout.hip) one site of the lazy row vector M_q[alpha, a] of <bits| W psi>, for nq rows packed per site:
//   X_q = M_q W[.. | s_out = sel[q * sel_step]] (chi_l x D_l) (D_l x 2 D_r),   M'_q = A^T X_q (chi_r x 2 chi_l) (2 chi_l x D_r)
// as two strided-batch GEMMs.  Wc / Ac are the call's scratch for the re-laid MPO site and the widened MPS site (Ac null when
// psi has the contraction dtype), X holds nq * chi_l 2 D_r elements.
int qil_lazy_row_step(qil_context* ctx, int dt, const struct qil_mpo* W, const struct qil_mps* psi, int64_t i, const void* Mc,
                      void* Mn, void* X, void* Wc, void* Ac, int64_t nq, const uint8_t* sel, int64_t sel_step);
// (qil_readout.hip) dout[t] = amplitude * v[t] (complex out, v of dtype dt), t < nb: the last step of a GEMM-form read-out
int qil_dev_finish_coeff(qil_context* ctx, int dt, const void* v, int64_t nb, double amplitude, void* dout);
// (qil_readout.hip) the read-out of nb rows of DEVICE bits (nb x n bytes, values 0 / 1 / 2) into dout (nb complex, device) under
// the marginal verb: its routes, CHAIN and GEMM_SELECT, need no host plan.  Only enqueues; temporaries go back in stream order.
int qil_coefficient_enqueue_select(const struct qil_mps* psi, int64_t nb, const uint8_t* dbits, void* dout);
// ---- (qil_index.hip) the wave-per-index reader: up to QIL_MAP_MAX_STATES chains of one length read at the same int64 device
// indices, the values (amplitudes included) optionally through an element-wise function (op = a QIL_MAP_* value, < 0: the value
// of state 0).  begin() uploads the site table into a block of tmp (stream-synchronised) and refuses a bond above what the LDS
// holds; enqueue() launches for `bound` indices or, with cnt_dev, for the device-side count *cnt_dev <= bound.  The carry dtype
// is c64 when any state is; out holds doubles for QIL_MAP_ABS / POWER / LOG and for all-real states, c64 otherwise.
constexpr int QIL_MAP_MAX_STATES = 4;
struct qil_index_reader {
    const void* tab = nullptr;
    int n = 0, nstates = 0, maxchi = 1;
    bool cx = false;
    double amp[QIL_MAP_MAX_STATES] = {};
};
int qil_index_reader_begin(qil_scratch& tmp, const struct qil_mps* const* states, int nstates, qil_index_reader* r);
int qil_index_reader_enqueue(qil_context* ctx, const qil_index_reader& r, int op, double param, const long long* idx,
                             const int* cnt_dev, int64_t bound, void* out);
// ---- (qil_cross.hip) the cross-interpolation session driven inside the library: cross_begin_impl, then per request
// eval(idx, cnt_dev, bound, vals) -- enqueue the evaluation of the *cnt_dev <= bound pending sample indices idx into vals
// (device, `dtype`) -- and cross_consume, then cross_finish_impl.  No host round trip per block.  Context active, call scope
// open, arguments checked (qil_cross_check_args: the ranges of qil_cross_begin under the caller's verb).
using qil_cross_eval = std::function<int(const long long* idx, const int* cnt_dev, long long bound, void* vals)>;
int qil_cross_check_args(const char* verb, qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps,
                         const int64_t* seeds, int64_t nseeds, const void* out);
int qil_cross_run(qil_context* ctx, int64_t n, int dtype, int64_t maxdim, double tol, int max_sweeps, const int64_t* seeds,
                  int64_t nseeds, const qil_cross_eval& eval, struct qil_mps** out, double* est, int64_t* nevals, int* sweeps,
                  int* converged);
// ---- (qil_contract.hip) the steps the overlap and Born-weight verbs share
// blocks of 256 threads for `work` items of a grid-stride kernel
inline unsigned qil_grid_for(long long work, long long cap = 4096) {
    return (unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, cap));
}
// p[t * stride] = 1 for t < count: the boundary [1] of an environment (count 1), the start of a batch of rows
int qil_dev_fill_ones(qil_context* ctx, int dt, void* p, int64_t count, int64_t stride = 1);
// Site i in the contraction dtype dt and the layout a product reads, into dst.  MPS A[s, sigma, beta]: PLAIN, REVERSED
// (Ap[beta, sigma, s]).  MPO W[a, s_in, s_out, b]: PLAIN, SWAPPED (Wp[a, s_out, s_in, b]), REVERSED (Wp[b, s_in, s_out, a]),
// REV_SWAPPED (Wp[b, s_out, s_in, a]), BIT_MAJOR (Wp[a, s_in, b, s_out]).
enum qil_site_layout { QIL_SITE_PLAIN = 0, QIL_SITE_SWAPPED = 1, QIL_SITE_REVERSED = 2, QIL_SITE_REV_SWAPPED = 3, QIL_SITE_BIT_MAJOR = 4 };
int qil_put_mps_site(qil_context* ctx, int dt, const struct qil_mps* psi, int64_t i, int layout, void* dst);
int qil_put_mpo_site(qil_context* ctx, int dt, const struct qil_mpo* W, int64_t i, int layout, void* dst);
// *use = site i of c as it lies when c has the dtype dt, else its PLAIN copy in buf
int qil_site_operand(qil_context* ctx, int dt, const struct qil_chain* c, int64_t i, void* buf, const void** use);
// The environment step of |W psi|^2 on nslots environments E[s', a', a, s] (cl Dl Dl cl each, packed), in two halves so that a
// caller can project T2 between them:  ket  T1 = E A (in -> s1), T2 = T1 W (s1 -> s2);  bra  T3 = T2 conj(Wr) (s2 -> s1),
// E' = A^H T3 (s1 -> out).  As, Wd: the sites in dt as they lie, Wr: the MPO site SWAPPED.  s2 may alias in and out.  The mirrored
// (right-to-left) step is the same call with cl <-> cr, Dl <-> Dr and the REVERSED / REV_SWAPPED operands.
int qil_norm_env_ket(qil_context* ctx, int dt, int64_t cl, int64_t cr, int64_t Dl, int64_t Dr, int64_t nslots, const void* As,
                     const void* Wd, const void* in, void* s1, void* s2);
int qil_norm_env_bra(qil_context* ctx, int dt, int64_t cl, int64_t cr, int64_t Dl, int64_t Dr, int64_t nslots, const void* As,
                     const void* Wr, const void* s2, void* s1, void* out);
inline int qil_norm_env_step(qil_context* ctx, int dt, int64_t cl, int64_t cr, int64_t Dl, int64_t Dr, int64_t nslots, const void* As,
                             const void* Wd, const void* Wr, const void* in, void* s1, void* s2, void* out) {
    QIL_TRY(qil_norm_env_ket(ctx, dt, cl, cr, Dl, Dr, nslots, As, Wd, in, s1, s2));
    return qil_norm_env_bra(ctx, dt, cl, cr, Dl, Dr, nslots, As, Wr, s2, s1, out);
}
// The environment step of <phi|psi>: T = E A_psi, E' = A_phi^H T with E (pl x sl), E' (pr x sr) column-major and ph physical slices
// per site (2 for states, 4 for operators); Ap, As: the sites in dt.  The mirrored (right-to-left) step is the same call with
// pl <-> pr, sl <-> sr and the REVERSED operands.
int qil_overlap_env_step(qil_context* ctx, int dt, int64_t ph, int64_t pl, int64_t pr, int64_t sl, int64_t sr, const void* Ap,
                         const void* As, const void* E, void* T, void* En);
// ... and of <phi|W psi>: T1 = E A_psi, T2_beta = T1_beta W, E' = A_phi^H T2 with E[p, a, s] (pl x Dl x sl); mirrored likewise
int qil_apply_overlap_env_step(qil_context* ctx, int dt, int64_t pl, int64_t pr, int64_t sl, int64_t sr, int64_t Dl, int64_t Dr,
                               const void* Ap, const void* As, const void* Wd, const void* E, void* T1, void* T2, void* En);
// (qil_inner.hip) phi against psi (or against W psi, which has psi's chain shape) for the overlap verbs: context, paired flag
// (QIL_EINVAL_ARG), length (QIL_EINVAL_LENGTH), site ids (QIL_EINVAL_SITES), under the name "inner"; touches no device
int qil_check_overlap_pair(const struct qil_mps* phi, const struct qil_mps* psi);
// `bytes` of caller memory into a new block of tmp (stream-synchronised: the source may go away when this returns)
int qil_upload_bytes(qil_scratch& tmp, const void* host, size_t bytes, void** dev);
// `bytes` of device memory to the caller, ordered after everything ctx has enqueued and complete on return (stream-synchronised)
int qil_download(qil_context* ctx, void* host_dst, const void* dev_src, size_t bytes);
// ---- (qil_apply_sample.hip) the two steps qil_apply_sample and qil_apply_top_k share
// bytes of right environments a call may keep (16 GiB, or QIL_APPLY_SAMPLE_RENV_BYTES, read on each call) and what (W, psi) needs
int64_t qil_apply_env_budget();
double qil_apply_env_bytes(const struct qil_mpo* W, const struct qil_mps* psi);
// the scoring route of a call: QIL_APPLY_SAMPLE_ROUTE, else the default for the largest product bond
bool qil_apply_score_fused(long long max_bond);
// partials per child and row that the fused route writes for a bond P: ceil(P / 64), the panels of its scoring kernel
int64_t qil_apply_score_panels(int64_t P);
// rows per chunk: max(1, min(rows, 32768, 64 MiB / per_row_bytes)), the budget of per-row temporaries and the batch limit of
// the row step's products
int64_t qil_apply_chunk_rows(int64_t rows, int64_t per_row_bytes);
// over the tensors: maxM = max(chi_l D_l, chi_r D_r) (a row vector), maxX = 2 chi_l D_r, maxW = 4 D_l D_r, maxA = 2 chi_l chi_r
struct qil_apply_bond_sizes {
    long long maxM = 1, maxX = 1, maxW = 1, maxA = 1;
};
qil_apply_bond_sizes qil_apply_sizes_of(const struct qil_mpo* W, const struct qil_mps* psi);
// ... from the n + 1 bond dimensions of the state and of the operator (readout_route has no handles)
qil_apply_bond_sizes qil_apply_sizes_of(int64_t n, const int64_t* chain_dims, const int64_t* op_dims);
// What a lazy sweep works with, all of it blocks of tmp: the site scratch of qil_lazy_row_step (Wc, and As where psi's dtype is
// not dt) and of the environment pass (At, Wd, Wr), the selector bytes {0, 1} (both + s: output bit s for every row of a step)
// and the environments Rk[1 .. n] (bond_k^2 elements, bond_k = chi_k D_k)
struct qil_apply_lazy {
    qil_apply_bond_sizes b;
    void *As = nullptr, *At = nullptr, *Wd = nullptr, *Wr = nullptr, *Wc = nullptr;
    const uint8_t* both = nullptr;
    std::vector<void*> Rk;
};
// The start of qil_apply_sample and qil_apply_top_k: fills lz, with the trace-normalised right environments of |W psi|^2 in the
// contraction dtype dt: Rk[n] = [1], Rk[k] = the mirrored four-product step of the scaled Rk[k + 1] divided by its trace t_k.
// *bad = 1 after a trace that is <= 0 or not finite (read back here); the caller reports it under its own name.  log_trace
// (nullable): *log_trace is a device double of tmp that receives sum_{k=0}^{n-1} log t_k = log |W psi|^2 without the amplitude,
// added up in tensor order by one workgroup; with a null log_trace nothing else changes.
int qil_apply_right_envs(qil_context* ctx, qil_scratch& tmp, int dt, const struct qil_mpo* W, const struct qil_mps* psi,
                         qil_apply_lazy& lz, int* bad, double** log_trace);
// Partial sums of q_s = Re(m_s R m_s^H) for both children of `rows` rows: child s of row r at children + (s rows + r) P,
// P = chi D, R the environment of that bond.  gemm route (fused = false): U (2 rows P elements) receives R^H [M_0 M_1] and
// *panels = 1; fused route: U is not used and *panels = ceil(P / 64).  part[(s *panels + panel) rows + r], to be summed in panel
// order.  Only enqueues.
int qil_apply_score_children(qil_context* ctx, int dt, bool fused, const void* children, int64_t rows, int64_t chi, int64_t D,
                             const void* R, void* U, double* part, int* panels);
// ---- (qil_topk.hip) the device-side selection qil_top_k and qil_apply_top_k share
// sel[0 .. M) = the positions of the M largest of the C non-negative keys (0 < M < C < 2^31), in ascending position; ties at the
// cut go to the lower position.  An MSD radix select on the keys' bit patterns, then a prefix-scan compaction.  state
// (qil_dev_select_state_bytes()) and blk (qil_dev_select_block_bytes(C)) are the caller's; dropmax (device, nullable) is
// raised to the bit pattern of the largest key that was not kept (an atomic max: the caller zeroes it once).  Only enqueues.
size_t qil_dev_select_state_bytes();
size_t qil_dev_select_block_bytes(long long C);
int qil_dev_select_largest(qil_context* ctx, const double* keys, long long C, long long M, int* sel, unsigned long long* dropmax,
                           void* state, void* blk);
// the k found rows (device order) to the caller in descending |value|, equal magnitudes in the device's order
void qil_top_k_deliver(int64_t k, int64_t n, const double* val, const uint8_t* bits, uint8_t* bits_out, double* val_out);
// ---- (qil_topk.hip) the beam search of qil_top_k and qil_apply_top_k
// The rows of a frontier, as the search sees them: row r of the f current rows has the children c = 2 r + s.  All pointers are
// device memory of the search; the calls only enqueue, and the search checks the launches.
struct qil_beam_rows {
    // both children of every row at site i: keys[c] and q[c] from p[r] (beam_keys, qil_device_utils.h)
    virtual int expand(int64_t i, long long f, const double* p, double* keys, double* q) = 0;
    // the M kept candidates sel[j] (j itself when sel is null) become the rows of site i + 1: gn, pn, anc by beam_gather_row
    virtual void gather(int64_t i, long long f, const double* keys, const double* q, const double* g, const int* sel, long long M,
                        double* gn, double* pn, int* anc) = 0;
    // the last site: val and bits of the M kept candidates by beam_finish_row
    virtual void finish(long long f, const double* g, const int* sel, long long M, const int* anc, long long stride, double lamp,
                        double sgn, double* val, uint8_t* bits) = 0;

protected:
    ~qil_beam_rows() = default;
};
long long qil_beam_frontier_cap(int64_t n, int64_t beam);   // the largest frontier: f_0 = 1, f_{i+1} = min(2 f_i, beam)
// The search over n sites from one row [1] (the caller's): per site expand, keep the min(2 f, beam) largest keys (min(2 f, k) at
// the last site), gather or finish; then the read-back, qil_top_k_deliver and the bound exp((log dropped + log_norm2) / 2) |amp|
// on the largest key dropped before the last site.  log_norm2: the host value, or with dev_log_norm2 the device double read back
// with the outputs.  The bookkeeping belongs to tmp.  One stream synchronisation, at the end.
int qil_beam_search(qil_context* ctx, qil_scratch& tmp, qil_beam_rows& rows, int64_t n, int64_t k, int64_t beam, double amp,
                    double log_norm2, const double* dev_log_norm2, uint8_t* bits_out, double* val_out, double* bound_out);
// (qil_hadamard.hip) phi against psi under `verb`: context, paired flag (QIL_EINVAL_ARG), length (QIL_EINVAL_LENGTH), site ids
// (QIL_EINVAL_SITES), in that order; touches no device
int qil_check_pair(const char* verb, const struct qil_mps* phi, const struct qil_mps* psi);
// (qil_inner.hip) the same four checks, in the same order and with the same codes, for two operators (qil_mpo_inner, qil_mpo_sum)
int qil_check_pair(const char* verb, const struct qil_mpo* V, const struct qil_mpo* W);
// (qil_apply.hip) the site table of the two fused-layout product kernels, site_apply_grouped and site_hadamard_grouped
// (qil_dev::ProductSite, qil_device_utils.h): result site i = left site i x right site i in row tiles of tile_rows, beta tiles of
// tb and left-bond chunks of nb.  Returns the workgroup count of the grouped grid.
namespace qil_dev {
struct ProductSite;
}
long long qil_product_sites(const qil_chain* left, const qil_chain* right, const qil_chain* out, int tile_rows, int tb, int nb,
                            std::vector<qil_dev::ProductSite>& tab);
// (qil_truncate.hip) the fused sum-and-truncate behind qil_mps_sum_compress: operands checked, context active, call scope open;
// w = nb (re, im) weights with the amplitudes folded in, odt = result dtype
int qil_sum_compress_impl(qil_context* ctx, const struct qil_mps* const* terms, int64_t nb, const double* w, int odt,
                          int64_t maxdim, double tol, int sweeps, int64_t zip_maxdim, struct qil_mps** out);
// (qil_truncate.hip) the exact gauge sweep of any chain (MPS or MPO) towards `center` (0 = the end of the direction): thin QR
// where the site is tall enough, the SVD at cut-off 0 otherwise; nothing is truncated.  Context active, call scope open.
int qil_gauge_exact(struct qil_chain* c, int direction, int64_t center);
// |r_jj|^2 (j < n <= 1024) of a triangular factor on the device, to the host
int qil_dev_diag_abs2(qil_context* ctx, int dtype, const void* R, int64_t ldr, int64_t n, double* host_out);
// At (n x m, ldt) = A^T (conj = 0) or A^H (conj = 1)
int qil_dev_transpose(qil_context* ctx, int dtype, int conj, int64_t m, int64_t n, const void* A, int64_t lda,
                      void* At, int64_t ldt);
// Thin SVD of A (m x n, lda) on the device: U (m x r0), S (r0, host), Vh (r0 x n), r0 = min(m,n).
// A is destroyed.  Singular values sorted descending.
// negligible_rel > 0: columns with |a|^2 < negligible_rel |A|_F^2 are left alone by the rotations (rounding residue
// of a rank-deficient operand; callers that truncate pass a value far below their cutoff).
int qil_dev_svd(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda, void* U,
                int64_t ldu, double* S_host, void* Vh, int64_t ldvh, double negligible_rel = 0.0);
// SVD with ONE isometric factor for the gauge sweeps: B (p x q; destroyed when *handled) = Uiso diag(S) V^H with
// Uiso (p x k, k = min(p, q)) orthonormal columns in descending-S order, SVh (k x q) = diag(S) V^H (no division by S
// anywhere).  Serves the mid-size regime (97 <= k < 640, and smaller operands that do not fit the single-workgroup iteration);
// *handled = 0 leaves B intact for the general qil_dev_svd.
// cert_cutoff > 0: the caller truncates by that cutoff only and ignores S_host; when the triangular factor certifies that no
// singular value can be dropped, the thin QR is returned as the gauge step (*handled = 2, S_host untouched).
// deflate > 0: rows of the triangular factor whose weight stays below deflate |B|_F^2 may be dropped (rank-deficient products).
int qil_dev_svd_left(qil_context* ctx, int dtype, int64_t p, int64_t q, void* B, int64_t ldb, void* Uiso, int64_t ldu,
                     double* S_host, void* SVh, int64_t ldsvh, double negligible_rel, int* handled, double cert_cutoff = 0.0,
                     double deflate = 0.0);
// The same certificate for operands of any size: thin QR of A (m >= n) or A^H (m < n) into Qout (max(m, n) x k, packed) and
// Rout (k x k, packed); *certified says whether a truncation at `cutoff` can drop anything.  A is left intact.
int qil_dev_qr_certified(qil_context* ctx, int dtype, int64_t m, int64_t n, const void* A, int64_t lda, double cutoff, void* Qout,
                         void* Rout, bool* certified);
// V (n x n, ldv) = I (the diagonal is written; the caller zeroes the rest)
int qil_dev_set_identity(qil_context* ctx, int dtype, void* V, int64_t ldv, int64_t n);
// Thin QR with non-negative real diagonal of R: A (m x n, m >= n) -> Q (m x n) in place; R (n x n) optional.
// orthonormal = true: Q^H Q is measured afterwards and Q re-factored while it is not the identity (numerically
// rank-deficient operands; one small GEMM and one stream synchronisation when nothing needs doing).
int qil_dev_qr_positive(qil_context* ctx, int dtype, int64_t m, int64_t n, void* A, int64_t lda,
                        void* R, int64_t ldr, bool orthonormal = false);
// device-to-device copies / zero fills as kernels (they ride the combined launches of a lock-step batch, qil_launch.h);
// pitches and widths in bytes
int qil_dev_copy2d(qil_context* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);
int qil_dev_copy(qil_context* ctx, void* dst, const void* src, size_t bytes);
int qil_dev_zero2d(qil_context* ctx, void* dst, size_t pitch, size_t width, size_t height);
int qil_dev_zero(qil_context* ctx, void* dst, size_t bytes);
// ITensors truncation rule (host): number of singular values kept.
int64_t qil_truncation_rank(const double* S, int64_t n, double cutoff, bool use_cutoff, int64_t maxdim,
                            int64_t mindim);
// scale columns (side=1: A[:, j] *= s[j]) or rows (side=0: A[i, :] *= s[i]) by real s (device copy made)
int qil_dev_scale(qil_context* ctx, int dtype, int side, int64_t m, int64_t n, void* A, int64_t lda,
                  const double* s_host);
int qil_dev_fill_normal(qil_context* ctx, int dtype, void* p, int64_t n_elems, uint64_t seed,
                        double scale);
