// Element-wise functions of states as new states: qil_mps_map.
//
// x -> f(psi_1[x], psi_2[x], ..) is not closed on MPS; it is cross-interpolated.  The session is the one of qil_signal_mps_cross
// (qil_cross_run, qil_cross.hip) with the gather from a dense signal replaced by the wave-per-index reader of qil_index.hip: one
// launch per block reads every operand at the block's sample indices (s->idx, count in CrossState::cnt) and applies f in its
// epilogue, writing the session's value buffer.  Nothing of a block crosses the host beyond what the session itself reads back.
#include "qil_internal.h"

#include <cmath>

namespace {

struct MapOp {
    const char* name;
    int nstates;
    bool has_param, positive;      // params[0]: required; > 0 (otherwise >= 0)
};
const MapOp kOps[] = {{"abs", 1, false, false}, {"power", 1, true, true}, {"log", 1, true, true}, {"divide", 2, true, false},
                      {"shrink", 1, true, false}};

}  // namespace

extern "C" int qil_mps_map(const qil_mps* const* states, int64_t nstates, int op, const double* params, int64_t maxdim, double tol,
                           int max_sweeps, const int64_t* seeds, int64_t nseeds, qil_mps** out, double* est, int64_t* nevals,
                           int* sweeps, int* converged) {
    QIL_REQUIRE(states && out, QIL_EINVAL_ARG, "map: null argument");
    QIL_REQUIRE(op >= QIL_MAP_ABS && op <= QIL_MAP_SHRINK, QIL_EINVAL_ARG, "map: unknown op %d", op);
    const MapOp& f = kOps[op];
    QIL_REQUIRE(nstates == f.nstates, QIL_EINVAL_ARG, "map: %s takes %d state%s, got nstates = %lld", f.name, f.nstates,
                f.nstates == 1 ? "" : "s", (long long)nstates);
    for (int64_t s = 0; s < nstates; ++s) QIL_REQUIRE(states[s], QIL_EINVAL_ARG, "map: null argument (states[%lld])", (long long)s);
    QIL_REQUIRE(!f.has_param || params, QIL_EINVAL_ARG, "map: null argument (params: %s takes a parameter)", f.name);
    const double param = f.has_param ? params[0] : 0.0;
    QIL_REQUIRE(std::isfinite(param) && (f.positive ? param > 0 : param >= 0), QIL_EINVAL_ARG, "map: params[0] = %g of %s must be finite and %s 0",
                param, f.name, f.positive ? ">" : ">=");
    // the ranges of the session's arguments before any handle is read (n = 62: the seeds' upper end follows below)
    QIL_TRY(qil_cross_check_args("map", reinterpret_cast<qil_context*>(const_cast<qil_mps**>(states)), 62, QIL_F64, maxdim, tol, max_sweeps,
                                 seeds, nseeds, out));
    const qil_mps* a = states[0];
    const int64_t n = a->n();
    QIL_REQUIRE(a->ctx, QIL_EINVAL_ARG, "map: null argument (a state without a context)");
    bool cx = false;
    for (int64_t s = 0; s < nstates; ++s) {
        const qil_mps* b = states[s];
        QIL_REQUIRE(b->ctx == a->ctx, QIL_EINVAL_ARG, "map: the states belong to different contexts");
        QIL_REQUIRE(!b->paired, QIL_EINVAL_ARG, "map: paired states are not supported; map the SignalMPS and call ztmps_from_mps");
        QIL_REQUIRE(b->n() == n, QIL_EINVAL_LENGTH, "map: the states must have the same number of sites. Found %lld and %lld",
                    (long long)n, (long long)b->n());
        QIL_REQUIRE(b->site_ids == a->site_ids, QIL_EINVAL_SITES, "map: the states must have the same site indices.");
        cx = cx || b->dtype == QIL_C64;
    }
    QIL_REQUIRE(n >= 1 && n <= 62, QIL_EINVAL_ARG, "map: %lld tensors outside 1 .. 62", (long long)n);
    for (int64_t t = 0; t < nseeds; ++t)
        QIL_REQUIRE(seeds[t] < (1LL << n), QIL_EINVAL_ARG, "map: seed %lld outside [0, 2^%lld)", (long long)seeds[t], (long long)n);
    const int odt = op <= QIL_MAP_LOG ? QIL_F64 : (cx ? QIL_C64 : QIL_F64);       // SHRINK has one operand: cx is its dtype
    *out = nullptr;
    qil_context* ctx = a->ctx;
    QIL_TRY(qil_ctx_activate(ctx));
    qil_call_scope call_scope(ctx);
    qil_scratch tmp(ctx);
    qil_index_reader reader;
    QIL_TRY(qil_index_reader_begin(tmp, states, (int)nstates, &reader));
    const qil_cross_eval eval = [&](const long long* idx, const int* cnt, long long bound, void* vals) {
        return qil_index_reader_enqueue(ctx, reader, op, param, idx, cnt, bound, vals);
    };
    qil_mps* res = nullptr;
    QIL_TRY(qil_cross_run(ctx, n, odt, maxdim, tol, max_sweeps, seeds, nseeds, eval, &res, est, nevals, sweeps, converged));
    res->site_ids = a->site_ids;
    *out = res;
    return QIL_OK;
}
