// epgx_run_check.cpp -- run analysis (epgx_run_check.h).  Plain C++17, no HIP.
#include "epgx_run_check.h"

#include <cstdlib>

namespace epgx {

int signal_room(const RunRequest &rq, bool exchange) {
    if (rq.naming) return EPGX_OK;
    const bool narrow = rq.signal_col0 < 0 || rq.signal_col0 + rq.nvox > rq.signal_ld;
    if (exchange) {
        if (!rq.has_signal || narrow) return fail(EPGX_ERR_INVALID, "epgx_run: range contains an ADC but the signal buffer is NULL or too narrow");
        return EPGX_OK;
    }
    if (!rq.has_signal) return fail(EPGX_ERR_INVALID, "epgx_run: range contains an ADC but signal is NULL");
    if (narrow)
        return fail(EPGX_ERR_INVALID, "epgx_run: signal columns [%lld,%lld) exceed signal_ld=%lld", (long long)rq.signal_col0,
                    (long long)(rq.signal_col0 + rq.nvox), (long long)rq.signal_ld);
    return EPGX_OK;
}

static int whole_groups(const PlanGeometry &geo, const RunRequest &rq) {
    if (rq.vox0 % geo.x_span || rq.nvox % geo.x_span)
        return fail(EPGX_ERR_INVALID, "epgx_run: voxel range [%lld,%lld) cuts compartment groups (blocks of %lld voxels)", (long long)rq.vox0,
                    (long long)(rq.vox0 + rq.nvox), (long long)geo.x_span);
    return EPGX_OK;
}

// A range that holds EPGX_OP_X in a plan with derivative states: ONE launch of dxrun_kernel<NC, M, V>, state and derivative
// states in registers, from equilibrium.  There is no split path for derivatives (the per-timestep derivative kernels keep no
// derivative states in HBM): what the kernel does not cover is EPGX_ERR_UNSUPPORTED.
static int analyse_exchange_deriv(const PlanHost &ph, const PlanGeometry &geo, const RunRequest &rq, RunDecision &d) {
    const int NC = d.NC, V = d.V = ph.n_vars, K = d.K;
    static const char *rule = "derivative states through an exchange (EPGX_OP_X) run on dxrun_kernel<N, K / 64, V>: N = 2 .. 4 compartments with "
                              "N * (K / 64) * (1 + V) <= 8, first order, from equilibrium (in = out = NULL), no D / gather shifts";
    if (ph.second) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: EPGX_DERIV_SECOND: %s", rule);
    if (rq.in.present || rq.out.present) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: a state in HBM: %s", rule);
    if (!xrun_deriv_fits(NC, K, V)) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: N = %d, K = %d, V = %d: %s", NC, K, V, rule);
    if (int rc = whole_groups(geo, rq)) return rc;
    for (int i = rq.op_begin; i < rq.op_end; ++i) {
        const int oc = ph.ops[i].opcode;
        if (oc == EPGX_OP_D || oc == EPGX_OP_GS) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: operator %d (opcode %d): %s", i, oc, rule);
        d.has_adc = d.has_adc || oc == EPGX_OP_ADC;
    }
    d.route = ROUTE_DXRUN;
    snprintf(d.name, sizeof(d.name), "dxrun_kernel<%d, %d, %d>", NC, d.M, V);
    return d.has_adc ? signal_room(rq, true) : EPGX_OK;
}

// A range that holds EPGX_OP_X.  xrun_kernel: one wavefront per group, NC = 2 .. 4 compartments, K = 64 .. 256 with
// NC * K / 64 <= 8, no D / gather shifts; everything else takes the split path.  The voxel range must hold whole groups.
static int analyse_exchange(const PlanHost &ph, const PlanGeometry &geo, const RunRequest &rq, const Knobs &kn, RunDecision &d) {
    const int K = d.K, NC = d.NC = geo.x_ncomp, M = d.M = K / 64;
    if (ph.n_vars > 0) return analyse_exchange_deriv(ph, geo, rq, d);
    if (!supported_K(K))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: ranges with an exchange (EPGX_OP_X) keep the state in HBM: K = 64 .. 1024, not %d", K);
    if (int rc = whole_groups(geo, rq)) return rc;
    bool fused = kn.xrun && NC >= 2 && NC <= 4 && K <= 256 && NC * M <= 8;
    // (the scan ends where the fused route does: behind it the pieces of the split path look after their own probes)
    for (int i = rq.op_begin; i < rq.op_end && fused; ++i) {
        fused = ph.ops[i].opcode != EPGX_OP_D && ph.ops[i].opcode != EPGX_OP_GS;
        d.has_adc = d.has_adc || ph.ops[i].opcode == EPGX_OP_ADC;
    }
    d.route = fused ? ROUTE_XRUN : ROUTE_XSPLIT;
    if (fused) snprintf(d.name, sizeof(d.name), "xrun_kernel<%d, %d, %s>", NC, M, rq.in.present ? "true" : "false");
    else snprintf(d.name, sizeof(d.name), "split<exchange_kernel>");
    return d.has_adc ? signal_room(rq, true) : EPGX_OK;
}

int analyse_run(const PlanHost &ph, const PlanGeometry &geo, const RunRequest &rq, const Knobs &kn, RunDecision *out) {
    RunDecision &d = *out;
    d = RunDecision();
    const int n_ops = (int)ph.ops.size();
    const int32_t op_begin = rq.op_begin, op_end = rq.op_end;
    const int64_t vox0 = rq.vox0, nvox = rq.nvox;
    if (op_begin < 0 || op_end > n_ops || op_begin > op_end)
        return fail(EPGX_ERR_INVALID, "epgx_run: operator range [%d,%d) outside [0,%d)", op_begin, op_end, n_ops);
    if (nvox > (int64_t)4 * 0x7fffffff) return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: more than 2^33 voxels in one launch");
    if (nvox < 0 || vox0 < 0 || vox0 + nvox > geo.nvox_total)
        return fail(EPGX_ERR_INVALID, "epgx_run: voxel range [%lld,%lld) outside the grid (%lld voxels)",
                    (long long)vox0, (long long)(vox0 + nvox), (long long)geo.nvox_total);
    const StateFacts &in = rq.in, &outs = rq.out;
    if (in.present && in.foreign) return fail(EPGX_ERR_INVALID, "epgx_run: `in` belongs to another context");
    if (outs.present && outs.foreign) return fail(EPGX_ERR_INVALID, "epgx_run: `out` belongs to another context");
    int K = rq.K;
    if (in.present) K = in.K;
    if (outs.present) {
        if (in.present && outs.K != in.K)
            return fail(EPGX_ERR_INVALID, "epgx_run: in/out capacities differ (%d vs %d)", in.K, outs.K);
        K = outs.K;
    }
    d.K = K;
    // K = 16: four voxels per wavefront (epgx_packed_kernels.hip.h), state-resident launches only
    const bool packed16 = d.packed16 = (K == 16 || K == 32);
    if (packed16 && (in.present || outs.present))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 keep no state in HBM: in and out must be NULL");
    // K = 2048: state-resident from equilibrium only (four wavefronts per voxel; a state matrix of that size has no HBM form)
    const bool wide = d.wide = K == 2048 && !in.present && !outs.present;
    if (!packed16 && !wide && !supported_K(K))
        return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K=%d not one of 16, 32, 2048 (state-resident only), 64, 128, 256, 512, 1024", K);
    if (in.present && in.nvox != nvox)
        return fail(EPGX_ERR_INVALID, "epgx_run: `in` holds %lld voxels, range has %lld", (long long)in.nvox,
                    (long long)nvox);
    if (outs.present && outs.nvox != nvox)
        return fail(EPGX_ERR_INVALID, "epgx_run: `out` holds %lld voxels, range has %lld", (long long)outs.nvox,
                    (long long)nvox);
    if (nvox == 0 || op_begin == op_end) {
        snprintf(d.name, sizeof(d.name), "none");
        return EPGX_OK;
    }

    bool has_x = false;
    for (int i = op_begin; i < op_end; ++i) {
        const epgx_op &op = ph.ops[i];
        has_x = has_x || op.opcode == EPGX_OP_X;
        if (op.opcode == EPGX_OP_S && std::abs(op.ia) >= K)
            return fail(EPGX_ERR_INVALID, "epgx_run: operator %d shifts by %d, capacity K=%d", i, op.ia, K);
        if (packed16 && (op.opcode == EPGX_OP_MAT || op.opcode == EPGX_OP_MAT0))
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: K = 16 / 32 do not handle general matrices (operator %d)", i);
        if (K == 32 && (op.opcode == EPGX_OP_D || op.opcode == EPGX_OP_GS))
            return fail(EPGX_ERR_UNSUPPORTED, "epgx_run: diffusion and gather shifts run with K = 16 or K >= 64 (operator %d)", i);
        if (op.opcode == EPGX_OP_D && op.ncoef != 3 * K)
            return fail(EPGX_ERR_INVALID, "epgx_run: operator %d: D table has %d doubles per entry, need 3*K=%d", i,
                        op.ncoef, 3 * K);
        if (op.opcode == EPGX_OP_GS) {
            if (2 * op.ncoef != 3 * K)
                return fail(EPGX_ERR_INVALID, "epgx_run: operator %d: gather table has %d entries, need 3*K=%d", i,
                            2 * op.ncoef, 3 * K);
            for (int32_t v : ph.gather_tables[i])
                if (v != -1 && ((v & ~(1 << 30)) < 0 || (v & ~(1 << 30)) >= K))
                    return fail(EPGX_ERR_INVALID, "epgx_run: operator %d: gather index %d outside [0,%d)", i, v, K);
        }
    }
    if (has_x) return analyse_exchange(ph, geo, rq, kn, d);
    d.route = ROUTE_RECORDS;
    return EPGX_OK;
}

int analyse_tiled(const char *who, bool deriv, const PlanHost &ph, const PlanGeometry &geo, int32_t Kbuf, int tiled_m, const TiledRequest *rq,
                  int32_t top0, TiledShape *out) {
    if (Kbuf < 64 || Kbuf % 64 != 0 || Kbuf > (1 << 24)) return fail(EPGX_ERR_INVALID, "%s: Kbuf=%d is not a multiple of 64 in [64, 2^24]", who, Kbuf);
    if (!deriv && ph.n_vars > 0)
        return fail(EPGX_ERR_UNSUPPORTED, "%s: plans with derivative states run at K <= 1024 (epgx_run)", who);
    if (deriv) {
        if (ph.second)
            return fail(EPGX_ERR_UNSUPPORTED, "%s: second-order plans (EPGX_DERIV_SECOND) run at K <= 512 (epgx_run)", who);
        if (ph.n_vars < 1 || ph.n_vars > TILED_DERIV_V)
            return fail(EPGX_ERR_UNSUPPORTED, "%s: the plan has %d derivative states, a launch carries 1 .. %d", who, ph.n_vars, TILED_DERIV_V);
    }
    for (size_t i = 0; i < ph.ops.size(); ++i) {
        const int oc = ph.ops[i].opcode;
        if (oc == EPGX_OP_X || oc == EPGX_OP_GS || oc == EPGX_OP_D)
            return fail(EPGX_ERR_UNSUPPORTED, "%s: operator %zu: exchange, gather shifts and diffusion run at K <= 1024 (epgx_run)", who, i);
    }
    if (rq) {
        const int64_t vox0 = rq->vox0, nvox = rq->nvox;
        const StateFacts &in = rq->in;
        if (nvox < 0 || vox0 < 0 || vox0 + nvox > geo.nvox_total)
            return fail(EPGX_ERR_INVALID, "%s: voxel range [%lld,%lld) outside the grid (%lld voxels)", who, (long long)vox0,
                        (long long)(vox0 + nvox), (long long)geo.nvox_total);
        if (rq->slab_voxels < 0) return fail(EPGX_ERR_INVALID, "%s: slab_voxels < 0", who);
        if (in.present) {
            if (in.foreign) return fail(EPGX_ERR_INVALID, "%s: `in` belongs to another context", who);
            if (in.nvox != nvox)
                return fail(EPGX_ERR_INVALID, "%s: `in` holds %lld voxels, range has %lld", who, (long long)in.nvox, (long long)nvox);
            if (in.K > 1024) return fail(EPGX_ERR_UNSUPPORTED, "%s: `in` has %d orders (at most 1024)", who, in.K);
            if (in.K > Kbuf) return fail(EPGX_ERR_INVALID, "%s: `in` has %d orders, Kbuf=%d", who, in.K, Kbuf);
        }
        top0 = in.present ? in.K - 1 : 0;
    } else if (top0 < 0 || top0 >= Kbuf)
        return fail(EPGX_ERR_INVALID, "%s: top0=%d outside [0, Kbuf)", who, top0);
    out->M = tiled_m == 16 && !deriv ? 16 : 8;
    out->H = out->M == 16 ? 64 : 32;
    out->top0 = top0;
    return EPGX_OK;
}

}  // namespace epgx
