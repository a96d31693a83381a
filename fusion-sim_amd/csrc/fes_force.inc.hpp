// fes_force.inc.hpp: the prescribed external forces of a CART3D handle (fpic_force, fpic_force_register, fpic_force_stats,
// fpic_force_clear) — part of fes_api.hip's translation unit (included there after fes_collide.inc.hpp, inside namespace fes).
// The rule and the checks of a request are fes_force_core.hpp, the pass fes_force_kernels.hpp.
//
// One launch per application over the range of pass_head (fes_ops.inc.hpp).  The family's rows (fes_ops.inc.hpp) hold fesforce::kWords tally words and room for three
// taper tables each.  A request's tables are copied at the call — the tapers to the device, the envelope to the host, where it
// is read once per application.  A registered request is enqueued by the hook with no host synchronisation and no
// collective; fpic_force_stats reads its row.  A force has no period: it is due at the sub-steps at which it is active.

constexpr int kForceNow = FPIC_FORCE_MAX_OPS;            // the row of fpic_force
constexpr size_t kForceTabDoubles = 3 * static_cast<size_t>(FPIC_FORCE_TABLE_MAX);   // per row

// a checked request into row `at`: its tally words zeroed, its taper tables on the device, the envelope in `op`
static int force_hold(fpic_handle* h, const fpic_force_spec& spec, int at, ForceOp& op)
{
    OpRows& rows = h->es->diag.force.rows;
    if (int rc = rows.room(h, fesforce::kWords, FPIC_FORCE_MAX_OPS + 1, kForceTabDoubles)) return rc;
    op.spec = spec;
    op.envelope.assign(spec.envelope, spec.envelope + spec.envelope_n);
    op.spec.envelope = nullptr;
    if (int rc = rows.zero(h, at)) return rc;
    double* tab = rows.table(at);
    bool any = false;
    for (int a = 0; a < 3; ++a) {
        op.taper[a] = nullptr;
        op.spec.taper[a] = nullptr;
        if (!spec.taper_n[a]) continue;
        HIP_TRY(h, hipMemcpyAsync(tab, spec.taper[a], spec.taper_n[a] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        op.taper[a] = tab;
        tab += spec.taper_n[a];
        any = true;
    }
    if (any) HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the caller's tables are pageable and may change after the call)
    return FPIC_OK;
}

// one application of `op` at s = `at` (the request is active there), its tallies added to `words`: enqueued, nothing waited for
template <typename T>
static int force_enqueue(fpic_handle* h, const ForceOp& op, uint64_t at, unsigned long long* words)
{
    State* st = h->es;
    const Species& sp = st->sp[op.spec.species];
    ForceArgs<T> a{};
    const unsigned grid = pass_head(h, sp, kForceBlocks, a);
    if (!grid) return FPIC_OK;
    const double L[3] = { st->lx, st->ly, st->lz };
    a.words = words;
    a.r = fesforce::rule_of(op.spec, L, sp.charge, sp.mass, h->spec.dt, at, op.envelope.data(), op.taper);
    if (a.r.whole && !a.r.tapered) {
        force_kernel<T, true><<<grid, kForceThreads, 0, h->stream>>>(a);
    } else {
        size_t lds = 0;
        for (int k = 0; k < 3; ++k) lds += op.spec.taper_n[k] * sizeof(double);
        force_kernel<T, false><<<grid, kForceThreads, lds, h->stream>>>(a);
    }
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int force_apply(fpic_handle* h, const ForceOp& op, uint64_t at, unsigned long long* words)
{
    return h->prec == FPIC_F32 ? force_enqueue<float>(h, op, at, words) : force_enqueue<double>(h, op, at, words);
}

static const char* force_check(fpic_handle* h, const fpic_force_spec* spec)
{
    const State* st = h->es;
    const double L[3] = { st->lx, st->ly, st->lz };
    return fesforce::check(spec, static_cast<int>(st->sp.size()), L);
}

int force(fpic_handle* h, const fpic_force_spec* spec, fpic_force_result* out)
{
    State* st = h->es;
    const OpRows& rows = st->diag.force.rows;
    if (const char* why = force_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_force_result{};
    const uint64_t at = st->diag.substep + spec->epoch;
    if (!fesforce::active(*spec, at)) return FPIC_OK;
    ForceOp op;
    if (int rc = force_hold(h, *spec, kForceNow, op)) return rc;
    if (int rc = force_apply(h, op, at, rows.row(kForceNow))) return rc;
    uint64_t got[fesforce::kWords] = {};
    if (int rc = rows.fetch(h, kForceNow, got)) return rc;
    if (out) {
        out->applications = 1;
        fesforce::result_of(got, st->sp[spec->species].mass, st->W, out);
    }
    return FPIC_OK;
}

int force_register(fpic_handle* h, const fpic_force_spec* spec, int* index)
{
    auto& f = h->es->diag.force;
    if (const char* why = force_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, fesops::kForce, 1)) return rc;
    ForceOp op;
    if (int rc = force_hold(h, *spec, static_cast<int>(f.ops.size()), op)) return rc;
    return ops_push(f, std::move(op), 1, index);
}

int force_stats(fpic_handle* h, int index, int scope, fpic_force_result* out)
{
    State* st = h->es;
    auto& f = st->diag.force;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kForce, index, scope, out, collective)) return rc;
    uint64_t got[fesforce::kWords] = {};
    if (int rc = f.rows.fetch(h, index, got)) return rc;
    if (collective) {
        uint64_t parts[fesforce::kSumWords];
        fesforce::split_words(got, parts);
        if (int rc = diag_sum_ranks(h, parts, fesforce::kSumWords)) return rc;
        fesforce::join_words(parts, got);
    }
    const ForceOp& op = f.ops[index];
    *out = fpic_force_result{};
    out->applications = op.applications;   // (the same on every rank: not summed)
    fesforce::result_of(got, st->sp[op.spec.species].mass, st->W, out);
    return FPIC_OK;
}

int force_clear(fpic_handle* h) { return ops_clear(h->es->diag.force); }

// the hook's part: every registered request that is active at s = the sub-step + its epoch (64 bits)
static int force_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.force;
    return ops_run_due<true>(f, [&](const ForceOp& op) { return fesforce::active(op.spec, substep + op.spec.epoch); },
                             [&](ForceOp& op, size_t k) { return force_apply(h, op, substep + op.spec.epoch, f.rows.row(k)); });
}
