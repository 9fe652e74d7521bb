// Host-only check of qil_scratch (qil_internal.h) against a stub pool.  Built by tests/test_scratch_handover.py with g++
// -fsanitize=address,undefined (the HIP headers on the include path, no device code, nothing linked from HIP): the ownership
// patterns of the calls that own their temporaries through it (inner_chain_route, inner_gemm_raw, qil_apply_inner, qil_apply_norm, lazy_gemm_path, upload_bits):
// every allocation may fail, every later step may fail, and each return path must free each block exactly once.
#include "qil_internal.h"

#include <cstdarg>
#include <cstdlib>
#include <set>

static std::set<void*> g_live;
static long g_allocs = 0, g_frees = 0, g_double = 0, g_fail_at = -1;

int qil_fail(int code, const char*, ...) { return code; }
int qil_ctx_alloc(qil_context*, size_t bytes, void** out) {
    if (g_fail_at >= 0 && g_allocs == g_fail_at) {
        ++g_allocs;
        return QIL_ENOMEM;
    }
    ++g_allocs;
    *out = malloc(bytes ? bytes : 1);
    g_live.insert(*out);
    return QIL_OK;
}
int qil_ctx_free(qil_context*, void* p) {
    if (!g_live.erase(p)) {
        ++g_double;              // a second free of the address (ASan would also flag the free() below)
        return QIL_EINVAL_ARG;
    }
    ++g_frees;
    free(p);
    return QIL_OK;
}

// the shape of inner_gemm_raw / qil_apply_inner / qil_apply_norm / lazy_gemm_path: up to 7 blocks, two of them optional, a loop of
// steps any of which may fail, no explicit free on the way out
static int contraction_call(qil_context* ctx, bool widen, int fail_step) {
    qil_scratch tmp(ctx);
    void* b[7] = {};
    for (int i = 0; i < 5; ++i) QIL_TRY(tmp.alloc(64 + 16 * i, &b[i]));
    if (widen) QIL_TRY(tmp.alloc(128, &b[5]));
    if (widen) QIL_TRY(tmp.alloc(256, &b[6]));
    for (int step = 0; step < 6; ++step) {
        if (step == fail_step) return qil_fail(QIL_EHIP, "step");
        memset(b[step % 5], step, 64);
    }
    return QIL_OK;
}
// the shape of qil_apply_coefficient_batch: upload_bits into the caller's scratch, then a callee with a scratch of its own; and of
// weigh(): blocks returned early (free), a block taken in from a callee (own) and one handed to the caller (give)
static int nested_call(qil_context* ctx, int fail_step, void** result) {
    qil_scratch tmp(ctx);
    void *bits = nullptr, *out = nullptr, *X = nullptr, *Y = nullptr, *theirs = nullptr;
    QIL_TRY(tmp.alloc(32, &bits));
    QIL_TRY(tmp.alloc(48, &out));
    QIL_TRY(tmp.alloc(512, &X));
    QIL_TRY(tmp.alloc(512, &Y));
    tmp.free(X);
    tmp.free(X);                                       // not ours any more: a second free must be a no-op
    QIL_TRY(contraction_call(ctx, true, fail_step));
    tmp.free(Y);
    QIL_TRY(qil_ctx_alloc(ctx, 96, &theirs));          // a callee's result
    tmp.own(theirs);
    if (fail_step == 100) return qil_fail(QIL_EHIP, "late");
    *result = tmp.give(out);                           // leaves the scratch: the caller frees it
    if (tmp.give(out) != nullptr) return qil_fail(QIL_EINVAL_ARG, "gave twice");
    return QIL_OK;
}

int main() {
    qil_context* ctx = nullptr;
    long calls = 0, failed = 0;
    for (int widen = 0; widen < 2; ++widen)
        for (int fail_step = -1; fail_step < 6; ++fail_step)
            for (g_fail_at = -1; g_fail_at < 8; ++g_fail_at) {
                g_allocs = 0;
                failed += contraction_call(ctx, widen != 0, fail_step) != QIL_OK;
                ++calls;
                if (!g_live.empty()) return printf("stranded after contraction_call(%d, %d, alloc %ld)\n", widen, fail_step, g_fail_at), 1;
            }
    for (int fail_step : {-1, 0, 3, 100})
        for (g_fail_at = -1; g_fail_at < 14; ++g_fail_at) {
            g_allocs = 0;
            void* result = nullptr;
            const int st = nested_call(ctx, fail_step, &result);
            failed += st != QIL_OK;
            ++calls;
            if (st == QIL_OK) {
                if (!result || g_live.size() != 1) return printf("hand-over lost its block\n"), 1;
                qil_ctx_free(ctx, result);
            }
            if (!g_live.empty()) return printf("stranded after nested_call(%d, alloc %ld)\n", fail_step, g_fail_at), 1;
        }
    printf("scratch_handover: %ld calls (%ld failed on purpose), %ld frees, %ld double frees\n", calls, failed, g_frees, g_double);
    return g_double == 0 ? 0 : 1;
}
