// fes_gas.inc.hpp: the windowed background collisions with a tabulated cross-section of a CART3D handle (fpic_gas,
// fpic_gas_register, fpic_gas_stats, fpic_gas_clear) — part of fes_api.hip's translation unit (included there after
// fes_force.inc.hpp, inside namespace fes).  The rule and the checks of a request are fes_gas_core.hpp, the pass
// fes_gas_kernels.hpp.
//
// One launch per application over the range of pass_head (fes_ops.inc.hpp).  The family's rows (fes_ops.inc.hpp) hold fesgas::kWords tally words and room for the
// cross-section table and three taper tables each.  A request's tables are copied at the call: to the device, and the cross-sections to the host too, where the candidate
// bound is formed.  Per request the host chooses which test the pass makes first (gas_window_first) and whether its
// candidates go through the LDS queue (gas_compacts); DESIGN 4.23 has the measurements behind the thresholds.  A registered
// operator is enqueued by the hook with no host synchronisation and no collective; fpic_gas_stats reads its row.
//
// TEST SWITCH (FPIC_GAS_FORMS, read once): which form runs, for measuring one against the other.  A sum of 1 (the word
// first), 2 (the window first), 4 (the wave-shared loop), 8 (the LDS queue); 0 or unset: the host's choices.  Every form
// gives the same particles.

constexpr int kGasNow = FPIC_GAS_MAX_OPS;                // the row of fpic_gas
constexpr size_t kGasTabDoubles = static_cast<size_t>(FPIC_GAS_TABLE_MAX) + 3 * static_cast<size_t>(FPIC_GAS_TAPER_MAX);   // per row

static int gas_forms()
{
    static const int forms = [] { const char* v = std::getenv("FPIC_GAS_FORMS"); return v ? std::atoi(v) : 0; }();
    return forms;
}

// a checked request into row `at`: its tally words zeroed, its tables on the device, the cross-sections in `op` too
static int gas_hold(fpic_handle* h, const fpic_gas_spec& spec, int at, GasOp& op)
{
    OpRows& rows = h->es->diag.gas.rows;
    if (int rc = rows.room(h, fesgas::kWords, FPIC_GAS_MAX_OPS + 1, kGasTabDoubles)) return rc;
    op.spec = spec;
    op.sigma.assign(spec.sigma, spec.sigma + spec.n);
    op.spec.sigma = nullptr;
    if (int rc = rows.zero(h, at)) return rc;
    double* tab = rows.table(at);
    HIP_TRY(h, hipMemcpyAsync(tab, op.sigma.data(), op.sigma.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    op.dev_sigma = tab;
    tab += spec.n;
    for (int a = 0; a < 3; ++a) {
        op.taper[a] = nullptr;
        op.spec.taper[a] = nullptr;
        if (!spec.taper_n[a]) continue;
        HIP_TRY(h, hipMemcpyAsync(tab, spec.taper[a], spec.taper_n[a] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        op.taper[a] = tab;
        tab += spec.taper_n[a];
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the tables are pageable and may change after the call)
    return FPIC_OK;
}

template <typename T, bool WINDOW_FIRST>
static void gas_launch(fpic_handle* h, const GasArgs<T>& a, unsigned grid, bool compact)
{
    if (compact) gas_kernel<T, WINDOW_FIRST, true><<<grid, kGasThreads, 0, h->stream>>>(a);
    else gas_kernel<T, WINDOW_FIRST, false><<<grid, kGasThreads, 0, h->stream>>>(a);
}

// one application of `op` at `epoch`, its tallies added to `words`: enqueued, nothing waited for
template <typename T>
static int gas_enqueue(fpic_handle* h, const GasOp& op, uint32_t epoch, unsigned long long* words)
{
    State* st = h->es;
    const Species& sp = st->sp[op.spec.species];
    const double L[3] = { st->lx, st->ly, st->lz };
    GasArgs<T> a{};
    const unsigned grid = pass_head(h, sp, kGasBlocks, a);
    a.r = fesgas::rule_of(op.spec, L, epoch, op.sigma.data(), op.dev_sigma, op.taper);
    if (!grid || a.r.K == 0) return FPIC_OK;   // (nothing can collide: nothing is launched)
    a.words = words;
    const int forms = gas_forms();
    const bool window_first = forms & 2 ? true : forms & 1 ? false : gas_window_first(a.r);
    const bool compact = forms & 8 ? true : forms & 4 ? false : gas_compacts(a.r.K);
    if (window_first) gas_launch<T, true>(h, a, grid, compact);
    else gas_launch<T, false>(h, a, grid, compact);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int gas_apply(fpic_handle* h, const GasOp& op, uint32_t epoch, unsigned long long* words)
{
    return h->prec == FPIC_F32 ? gas_enqueue<float>(h, op, epoch, words) : gas_enqueue<double>(h, op, epoch, words);
}

static const char* gas_check(fpic_handle* h, const fpic_gas_spec* spec)
{
    const State* st = h->es;
    const double L[3] = { st->lx, st->ly, st->lz };
    return fesgas::check(spec, static_cast<int>(st->sp.size()), L);
}

int gas(fpic_handle* h, const fpic_gas_spec* spec, fpic_gas_result* out)
{
    State* st = h->es;
    const OpRows& rows = st->diag.gas.rows;
    if (const char* why = gas_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_gas_result{};
    const double p_max = -std::expm1(-fesgas::x_max_of(*spec));
    if (static_cast<uint64_t>(std::ldexp(p_max, 32)) == 0) return FPIC_OK;   // (K = 0: nothing is launched, nothing is held)
    GasOp op;
    if (int rc = gas_hold(h, *spec, kGasNow, op)) return rc;
    if (int rc = gas_apply(h, op, spec->epoch, rows.row(kGasNow))) return rc;
    uint64_t got[fesgas::kWords] = {};
    if (int rc = rows.fetch(h, kGasNow, got)) return rc;
    if (out) {
        out->applications = 1;
        fesgas::result_of(got, st->sp[spec->species].mass, st->W, out);
    }
    return FPIC_OK;
}

int gas_register(fpic_handle* h, const fpic_gas_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.gas;
    if (const char* why = gas_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, fesops::kGas, every)) return rc;
    GasOp op;
    if (int rc = gas_hold(h, *spec, static_cast<int>(f.ops.size()), op)) return rc;
    return ops_push(f, std::move(op), every, index);
}

int gas_stats(fpic_handle* h, int index, int scope, fpic_gas_result* out)
{
    State* st = h->es;
    auto& f = st->diag.gas;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kGas, index, scope, out, collective)) return rc;
    uint64_t got[fesgas::kWords] = {};
    if (int rc = f.rows.fetch(h, index, got)) return rc;
    if (collective) {
        uint64_t parts[fesgas::kSumWords];
        fesgas::split_words(got, parts);
        if (int rc = diag_sum_ranks(h, parts, fesgas::kSumWords)) return rc;
        fesgas::join_words(parts, got);
    }
    const GasOp& op = f.ops[index];
    *out = fpic_gas_result{};
    out->applications = op.applications;   // (the same on every rank: not summed)
    fesgas::result_of(got, st->sp[op.spec.species].mass, st->W, out);
    return FPIC_OK;
}

int gas_clear(fpic_handle* h) { return ops_clear(h->es->diag.gas); }

// the hook's part: every registered operator that is due, at the epoch of the sub-step
static int gas_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.gas;
    return ops_run_due<true>(f, OpsEvery{ substep }, [&](GasOp& op, size_t k) { return gas_apply(h, op, static_cast<uint32_t>(substep + op.spec.epoch), f.rows.row(k)); });
}
