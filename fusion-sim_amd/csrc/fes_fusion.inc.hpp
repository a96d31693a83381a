// fes_fusion.inc.hpp: the fusion yield tally of a CART3D handle (fpic_fusion, fpic_fusion_register, fpic_fusion_stats,
// fpic_fusion_grid, fpic_fusion_clear) — part of fes_api.hip's translation unit (included there after fes_pair.inc.hpp, inside
// namespace fes).  The rule and the checks of a request are fes_fusion_core.hpp, the pass fes_fusion_kernels.hpp.
//
// One application: per species of the request fpic_pair's cell index (pair_index<T>, into the Diag's index buffers,
// unchanged), then the tally pass — all enqueued on the handle's stream, nothing read back.  The family's rows
// (fes_ops.inc.hpp) hold eight count words and a table each (the tables an allocation of their own); beside every row the
// Diag keeps a cell grid, allocated when the row is first used.  A table is uploaded at the call or at the registration (which
// waits for the copy: the caller's table need not outlive it); the hook never allocates and never waits.
// A handle with a Domain is refused as fpic_pair refuses it.

constexpr int kFusionWords = 8;                     // per row: pairs, below, above, cells, overfull_cells, overfull_particles, yield_hi, yield_lo
constexpr int kFusionNow = FPIC_FUSION_MAX_OPS;     // the row of fpic_fusion

// the row starts from zero with the request's table, in stream order; returns after the table has been copied
static int fusion_begin(fpic_handle* h, int slot, const fpic_fusion_spec& spec)
{
    State* st = h->es;
    Diag& g = st->diag;
    OpRows& rows = g.fusion.rows;
    const size_t grid_bytes = pair_cells(st) * sizeof(unsigned long long);
    if (int rc = rows.room(h, kFusionWords, FPIC_FUSION_MAX_OPS + 1, FPIC_FUSION_TABLE_MAX, true)) return rc;
    if (!g.fusion_grid[slot])
        if (int rc = dev_alloc(h, reinterpret_cast<void**>(&g.fusion_grid[slot]), grid_bytes, &h->bytes_grid)) return rc;
    if (int rc = rows.zero(h, slot)) return rc;
    HIP_TRY(h, hipMemsetAsync(g.fusion_grid[slot], 0, grid_bytes, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rows.table(slot), spec.sigma, static_cast<size_t>(spec.n) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

// the index buffers of the request's species, as fpic_pair sizes them
static int fusion_buffers(fpic_handle* h, const fpic_fusion_spec& spec, bool may_grow)
{
    fpic_pair_spec p{};
    p.species_a = spec.species_a;
    p.species_b = spec.species_b;
    return pair_buffers(h, p, may_grow);
}

// one application of the rule r into `slot`: enqueued, nothing waited for
template <typename T>
static int fusion_enqueue(fpic_handle* h, const fpic_fusion_spec& spec, const fesfusion::Rule& r, int slot, bool may_grow)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = fusion_buffers(h, spec, may_grow)) return rc;
    const Species& sa = st->sp[spec.species_a];
    const Species& sb = st->sp[spec.species_b];
    const bool like = spec.species_a == spec.species_b;
    if (!sa.n || !sb.n || !(r.s_max > 0)) return FPIC_OK;   // (nothing can react: nothing is launched)
    if (int rc = pair_index<T>(h, sa, 0)) return rc;
    if (!like)
        if (int rc = pair_index<T>(h, sb, 1)) return rc;
    FusionArgs<T> a{};
    const unsigned grid = pair_head(st, sa, sb, a);
    a.counts = g.fusion.rows.row(slot);
    a.grid = g.fusion_grid[slot];
    a.table = g.fusion.rows.table(slot);
    a.r = r;
    // (kFusionLdsBytes is below the 64 KiB a launch may ask for without an attribute: the header asserts it)
    if (like) fusion_tally_kernel<T, true><<<grid, kPairThreads, kFusionLdsBytes, h->stream>>>(a);
    else fusion_tally_kernel<T, false><<<grid, kPairThreads, kFusionLdsBytes, h->stream>>>(a);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int fusion_apply(fpic_handle* h, const fpic_fusion_spec& spec, const fesfusion::Rule& r, int slot, bool may_grow)
{
    return h->prec == FPIC_F32 ? fusion_enqueue<float>(h, spec, r, slot, may_grow) : fusion_enqueue<double>(h, spec, r, slot, may_grow);
}

static double fusion_dv(const State* st) { return (st->lx / st->nx) * (st->ly / st->ny) * (st->lz / st->nz); }

static int fusion_check(fpic_handle* h, const fpic_fusion_spec* spec)
{
    State* st = h->es;
    if (const char* why = fesfusion::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fesfusion::check_bound(*spec, st->W, fusion_dv(st))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}

static void fusion_result(fpic_fusion_result* out, uint64_t applications, const uint64_t* got, int e)
{
    *out = fpic_fusion_result{};
    out->applications = applications;
    out->pairs = got[0];
    out->below = got[1];
    out->above = got[2];
    out->cells = got[3];
    out->overfull_cells = got[4];
    out->overfull_particles = got[5];
    uint64_t hi, lo;
    fesfusion::join(got[6], got[7], hi, lo);
    out->yield_hi = hi;
    out->yield_lo = lo;
    out->unit_exponent = e;
}

int fusion(fpic_handle* h, const fpic_fusion_spec* spec, fpic_fusion_result* out, int64_t* grid)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion")) return rc;
    if (int rc = fusion_check(h, spec)) return rc;
    if (out) *out = fpic_fusion_result{};
    if (int rc = fusion_begin(h, kFusionNow, *spec)) return rc;
    const fesfusion::Rule r = fesfusion::rule_of(*spec, spec->epoch, st->W, fusion_dv(st));
    if (int rc = fusion_apply(h, *spec, r, kFusionNow, true)) return rc;
    uint64_t got[kFusionWords] = {};
    if (grid) HIP_TRY(h, hipMemcpyAsync(grid, g.fusion_grid[kFusionNow], pair_cells(st) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (int rc = g.fusion.rows.fetch(h, kFusionNow, got)) return rc;
    if (out) fusion_result(out, 1, got, r.e);
    return FPIC_OK;
}

int fusion_register(fpic_handle* h, const fpic_fusion_spec* spec, int every, int* index)
{
    State* st = h->es;
    auto& f = st->diag.fusion;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_register")) return rc;
    if (int rc = fusion_check(h, spec)) return rc;
    if (int rc = ops_check_register(h, f, fesops::kFusion, every)) return rc;
    if (int rc = fusion_buffers(h, *spec, true)) return rc;   // (sized now: the hook finds them in place and never grows them)
    if (int rc = fusion_begin(h, static_cast<int>(f.ops.size()), *spec)) return rc;
    FusionOp op;
    op.spec = *spec;
    op.spec.sigma = nullptr;        // (the table is on the device; the caller's need not outlive this call)
    op.rule = fesfusion::rule_of(*spec, spec->epoch, st->W, fusion_dv(st));
    return ops_push(f, op, every, index);
}

int fusion_stats(fpic_handle* h, int index, int scope, fpic_fusion_result* out)
{
    auto& f = h->es->diag.fusion;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kFusion, index, scope, out, collective)) return rc;
    uint64_t got[kFusionWords] = {};
    if (int rc = f.rows.fetch(h, index, got)) return rc;
    if (collective)
        if (int rc = diag_sum_ranks(h, got, kFusionWords)) return rc;
    fusion_result(out, f.ops[index].applications, got, f.ops[index].rule.e);
    return FPIC_OK;
}

int fusion_grid(fpic_handle* h, int index, int64_t* grid, int reset)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_grid")) return rc;
    if (int rc = ops_check_index(h, g.fusion, fesops::kFusion, index)) return rc;
    if (!grid && !reset) return fail(h, FPIC_ERR_INVALID_ARG, ".grid <- Non-optional property is undefined!");
    const size_t bytes = pair_cells(st) * sizeof(int64_t);
    if (grid) HIP_TRY(h, hipMemcpyAsync(grid, g.fusion_grid[index], bytes, hipMemcpyDeviceToHost, h->stream));
    if (reset) {   // (behind the copy, in stream order)
        HIP_TRY(h, hipMemsetAsync(g.fusion_grid[index], 0, bytes, h->stream));
        if (int rc = g.fusion.rows.zero(h, index)) return rc;
        g.fusion.ops[index].applications = 0;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

int fusion_clear(fpic_handle* h)
{
    if (int rc = pair_refuse_decomposed(h, "fpic_fusion_clear")) return rc;
    return ops_clear(h->es->diag.fusion);
}

// the hook's part: every registered tally that is due — the registered rule at the epoch of the sub-step; nothing grows here
static int fusion_after_substep(fpic_handle* h, uint64_t substep)
{
    return ops_run_due<true>(h->es->diag.fusion, OpsEvery{ substep }, [&](FusionOp& op, size_t k) {
        fesfusion::Rule r = op.rule;
        r.epoch = static_cast<uint32_t>(substep + op.spec.epoch);
        return fusion_apply(h, op.spec, r, static_cast<int>(k), false);
    });
}
