// fes_ionize.inc.hpp: the electron-impact ionisation of a background gas of a CART3D handle (fpic_ionize,
// fpic_ionize_register, fpic_ionize_stats, fpic_ionize_clear) — part of fes_api.hip's translation unit (included there after
// fes_inject.inc.hpp, inside namespace fes).  The rule and the checks of a request are fes_ionize_core.hpp, the passes
// fes_ionize_kernels.hpp.
//
// One application: the deciding pass over the projectile species (it writes the counts into the application's row, the event
// list, the bitmap of the primaries' ids and the cursor — no particle state), and ONE 8-byte copy back that the host waits
// for — the event count M: the host has to learn the new n, also in the hook.  M = 0: the counts are added to the ioniser's
// totals and nothing else happens.  Else the host holds M against both targets' capacities and id bounds and refuses before
// anything has changed (the totals included: the application's row is a row of its own).  Then the popcount scan of the
// bitmap (fpic_renumber's kernels), the generation pass over the M events, the add of the application's row to the totals,
// and for each target the state a source leaves (species_appended, fes_inject.inc.hpp).  The electrostatic re-deposit is inject_settle: once per call, and once
// per sub-step after the last ioniser that is due — the sources due on the same sub-step have settled before (the hook runs
// the families one after the other; sharing the re-deposit would make the sources' part wait for a family behind it).
//
// The buffers of an application lie in the selection's buffer (select_buffer: it grows to the largest request and is counted
// in bytes_grid; every user of it is synchronous): the bitmap over the projectile's id span, per word the marked ids below it
// in its chunk, the chunks' counts, the scan's total, the cursor, the event list (8 bytes per live projectile).  The id span
// is read per application, so a source that has raised it since the registration is followed.
//
// TEST SWITCH (FPIC_IONIZE_FORMS, read once): which form of the deciding pass runs, as FPIC_GAS_FORMS: a sum of 1 (the word
// first), 2 (the window first), 4 (the wave-shared loop), 8 (the LDS queue); 0 or unset: the host's choices (gas_window_first,
// gas_compacts: the gas pass's thresholds).  Every form gives the same particles.

constexpr int kIonizeNow = FPIC_IONIZE_MAX_OPS;          // the row of the application in flight (and of fpic_ionize's tables)

// the noun is the family's own: the shared table (fes_ops_core.hpp) keeps the eight families it was written for
static const fesops::Messages kIonizeMessages = { FPIC_IONIZE_MAX_OPS, ".spec <- FPIC_IONIZE_MAX_OPS (8) ionisers are registered already", ".index <- no such registered ioniser" };

static int ionize_forms()
{
    static const int forms = [] { const char* v = std::getenv("FPIC_IONIZE_FORMS"); return v ? std::atoi(v) : 0; }();
    return forms;
}

// a checked request into the table room of row `at`: its tables on the device, the cross-sections in `op` too
static int ionize_hold(fpic_handle* h, const fpic_ionize_spec& spec, int at, IonizeOp& op)
{
    OpRows& rows = h->es->diag.ionize.rows;
    if (int rc = rows.room(h, fesion::kWords, FPIC_IONIZE_MAX_OPS + 1, kGasTabDoubles)) return rc;
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
static void ionize_launch(fpic_handle* h, const IonizeDecideArgs<T>& a, unsigned grid, bool compact)
{
    if (compact) ionize_decide_kernel<T, WINDOW_FIRST, true><<<grid, kGasThreads, 0, h->stream>>>(a);
    else ionize_decide_kernel<T, WINDOW_FIRST, false><<<grid, kGasThreads, 0, h->stream>>>(a);
}

// One application of `op` at `epoch`: the application's row into row kIonizeNow, added to row `total_row` (< 0: to none);
// *events = M.  hook: a request that does not fit is a state error there.  Not settled (inject_settle is the caller's, if M).
template <typename T>
static int ionize_run(fpic_handle* h, const IonizeOp& op, uint32_t epoch, int total_row, bool hook, uint64_t* events)
{
    State* st = h->es;
    Diag& g = st->diag;
    const fpic_ionize_spec& spec = op.spec;
    Species& sp = st->sp[spec.species];
    Species& se = st->sp[spec.electron];
    Species& si = st->sp[spec.ion];
    const OpRows& rows = g.ionize.rows;
    *events = 0;
    if (int rc = rows.zero(h, kIonizeNow)) return rc;
    const double L[3] = { st->lx, st->ly, st->lz };
    IonizeDecideArgs<T> a{};
    const unsigned grid = pass_head(h, sp, kGasBlocks, a);
    a.r = fesion::rule_of(spec, L, epoch, op.sigma.data(), op.dev_sigma, op.taper);
    if (!grid || a.r.g.K == 0) return FPIC_OK;   // (nothing can ionise: nothing is launched)
    // the buffers: bitmap | below | chunk counts | the scan's total, the cursor | the event list
    const uint64_t span = id_span_of(sp);
    const size_t nwords = static_cast<size_t>((span + 31) / 32), nchunks = (nwords + kRenumberChunk - 1) / kRenumberChunk;
    const size_t below_at = (nwords * sizeof(uint32_t) + 15) / 16 * 16, chunk_at = 2 * below_at, total_at = chunk_at + (nchunks * sizeof(uint32_t) + 15) / 16 * 16;
    const size_t events_at = total_at + 16;
    if (int rc = select_buffer(h, events_at + a.s1 * sizeof(IonizeEvent))) return rc;
    unsigned char* dev = static_cast<unsigned char*>(g.sel);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(dev);
    uint32_t* below = reinterpret_cast<uint32_t*>(dev + below_at);
    uint32_t* chunk = reinterpret_cast<uint32_t*>(dev + chunk_at);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(dev + total_at);
    HIP_TRY(h, hipMemsetAsync(bitmap, 0, nwords * sizeof(uint32_t), h->stream));
    HIP_TRY(h, hipMemsetAsync(total, 0, 16, h->stream));
    a.words = rows.row(kIonizeNow);
    a.cursor = total + 1;
    a.events = reinterpret_cast<IonizeEvent*>(dev + events_at);
    a.bitmap = bitmap;
    const int forms = ionize_forms();
    const bool window_first = forms & 2 ? true : forms & 1 ? false : gas_window_first(a.r.g);
    const bool compact = forms & 8 ? true : forms & 4 ? false : gas_compacts(a.r.g.K);
    if (window_first) ionize_launch<T, true>(h, a, grid, compact);
    else ionize_launch<T, false>(h, a, grid, compact);
    HIP_TRY(h, hipGetLastError());
    unsigned long long got = 0;
    HIP_TRY(h, hipMemcpyAsync(&got, a.cursor, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (got > a.s1) return fail(h, FPIC_ERR_HIP, "fpic_ionize counted %llu events among %zu particles", got, a.s1);
    unsigned long long* const totals = total_row < 0 ? nullptr : rows.row(total_row);
    if (!got) {   // no event: the counts, and nothing else changes
        if (totals) ionize_add_kernel<<<1, 1, 0, h->stream>>>(rows.row(kIonizeNow), totals);
        HIP_TRY(h, hipGetLastError());
        return FPIC_OK;
    }
    // (electron == species: se is sp, the same numbers)
    const uint64_t span_e = id_span_of(se), span_i = id_span_of(si);
    if (const char* who = fesion::fit(got, se.n, se.cap, span_e, si.n, si.cap, span_i)) {
        const bool e = who[0] == 'e';
        const Species& t = e ? se : si;
        return fail(h, hook ? FPIC_ERR_STATE : FPIC_ERR_INVALID_ARG,
                    ".%s <- species %d holds %zu particles (ids below %llu) of a capacity of %zu: the %llu of this application do not fit; call fpic_reserve first; nothing was changed",
                    who, e ? spec.electron : spec.ion, t.n, static_cast<unsigned long long>(e ? span_e : span_i), t.cap, got);
    }
    renumber_count_kernel<<<static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (nchunks + 3) / 4)), 256, 0, h->stream>>>(bitmap, nwords, below, chunk, nchunks);
    load_scan_kernel<<<1, 1024, 0, h->stream>>>(chunk, nchunks, total);
    IonizeGenerateArgs<T> q{};
    q.slab = a.slab;
    q.n_pad = a.n_pad;
    q.events = a.events;
    q.m = static_cast<uint32_t>(got);
    q.bitmap = bitmap;
    q.below = below;
    q.offset = chunk;
    q.slab_e = static_cast<T*>(se.slab[se.cur]);
    q.n_pad_e = se.n_pad;
    q.id_e = se.id[se.cur];
    q.s0_e = se.n;
    q.id0_e = static_cast<uint32_t>(span_e);
    q.slab_i = static_cast<T*>(si.slab[si.cur]);
    q.n_pad_i = si.n_pad;
    q.id_i = si.id[si.cur];
    q.s0_i = si.n;
    q.id0_i = static_cast<uint32_t>(span_i);
    q.words = rows.row(kIonizeNow) + fesion::kCounts;
    q.r = a.r;
    const unsigned ggrid = static_cast<unsigned>(std::min<size_t>(kIonizeBlocks, (static_cast<size_t>(got) + kIonizeThreads - 1) / kIonizeThreads));
    ionize_generate_kernel<T><<<ggrid, kIonizeThreads, 0, h->stream>>>(q);
    if (totals) ionize_add_kernel<<<1, 1, 0, h->stream>>>(rows.row(kIonizeNow), totals);
    HIP_TRY(h, hipGetLastError());
    if (int rc = species_appended(h, se, span_e, got)) return rc;
    if (int rc = species_appended(h, si, span_i, got)) return rc;
    *events = got;
    return FPIC_OK;
}

static int ionize_apply(fpic_handle* h, const IonizeOp& op, uint32_t epoch, int total_row, bool hook, uint64_t* events)
{
    return h->prec == FPIC_F32 ? ionize_run<float>(h, op, epoch, total_row, hook, events) : ionize_run<double>(h, op, epoch, total_row, hook, events);
}

static const char* ionize_check(fpic_handle* h, const fpic_ionize_spec* spec)
{
    const State* st = h->es;
    const double L[3] = { st->lx, st->ly, st->lz };
    return fesion::check(spec, static_cast<int>(st->sp.size()), L);
}

static int ionize_fetch(fpic_handle* h, int row, const fpic_ionize_spec& spec, fpic_ionize_result* out)
{
    State* st = h->es;
    uint64_t got[fesion::kWords] = {};
    if (int rc = st->diag.ionize.rows.fetch(h, row, got)) return rc;
    const Species &sp = st->sp[spec.species], &se = st->sp[spec.electron], &si = st->sp[spec.ion];
    const double mass[3] = { sp.mass, se.mass, si.mass }, charge[3] = { sp.charge, se.charge, si.charge };
    fesion::result_of(got, mass, charge, st->W, out);
    return FPIC_OK;
}

int ionize(fpic_handle* h, const fpic_ionize_spec* spec, fpic_ionize_result* out)
{
    if (int rc = inject_refuse_decomposed(h, "fpic_ionize")) return rc;
    if (const char* why = ionize_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_ionize_result{};
    const double p_max = -std::expm1(-fesion::x_max_of(*spec));
    if (static_cast<uint64_t>(std::ldexp(p_max, 32)) == 0) return FPIC_OK;   // (K = 0: nothing is launched, nothing is held)
    IonizeOp op;
    if (int rc = ionize_hold(h, *spec, kIonizeNow, op)) return rc;
    uint64_t events = 0;
    if (int rc = ionize_apply(h, op, spec->epoch, -1, false, &events)) return rc;
    if (events)
        if (int rc = inject_settle(h)) return rc;
    if (!out) return FPIC_OK;
    if (int rc = ionize_fetch(h, kIonizeNow, *spec, out)) return rc;
    out->applications = 1;
    return FPIC_OK;
}

int ionize_register(fpic_handle* h, const fpic_ionize_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.ionize;
    if (int rc = inject_refuse_decomposed(h, "fpic_ionize_register")) return rc;
    if (const char* why = ionize_check(h, spec)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, kIonizeMessages, every)) return rc;
    IonizeOp op;
    if (int rc = ionize_hold(h, *spec, static_cast<int>(f.ops.size()), op)) return rc;
    return ops_push(f, std::move(op), every, index);
}

int ionize_stats(fpic_handle* h, int index, int scope, fpic_ionize_result* out)
{
    auto& f = h->es->diag.ionize;
    if (int rc = inject_refuse_decomposed(h, "fpic_ionize_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, kIonizeMessages, index, scope, out, collective)) return rc;   // (undecomposed: GLOBAL is LOCAL)
    const IonizeOp& op = f.ops[index];
    *out = fpic_ionize_result{};
    if (int rc = ionize_fetch(h, index, op.spec, out)) return rc;
    out->applications = op.applications;
    return FPIC_OK;
}

int ionize_clear(fpic_handle* h)
{
    if (int rc = inject_refuse_decomposed(h, "fpic_ionize_clear")) return rc;
    return ops_clear(h->es->diag.ionize);   // (every application has ended synchronised: nothing is in flight)
}

// the hook's part: every registered ioniser that is due, at the epoch of the sub-step, counted once it has succeeded; each
// waits for its event count.  Then ONE re-deposit and solve for all of them that had events (inject_settle).  An ioniser that
// fails leaves what the ones before it did, settled.
static int ionize_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.ionize;
    bool grown = false;
    int rc = ops_run_due<false>(f, OpsEvery{ substep }, [&](IonizeOp& op, size_t k) {
        uint64_t events = 0;
        const int e = ionize_apply(h, op, static_cast<uint32_t>(substep + op.spec.epoch), static_cast<int>(k), true, &events);
        if (events) grown = true;
        return e;
    });
    if (grown) {
        const std::string why = h->err;          // (the settling must not lose the message of the ioniser that failed)
        const int settled = inject_settle(h);
        if (rc != FPIC_OK) h->err = why;
        else rc = settled;
    }
    return rc;
}
