// fes_burn.inc.hpp: the fusion burn of a CART3D handle (fpic_burn, fpic_burn_register, fpic_burn_stats, fpic_burn_clear) —
// part of fes_api.hip's translation unit (included there after fes_ionize.inc.hpp, inside namespace fes).  The rule and the
// checks of a request are fes_burn_core.hpp, the passes fes_burn_kernels.hpp.
//
// One application: per reactant species fpic_pair's cell index (pair_index<T>, unchanged), the deciding pass (it writes the
// counts into the application's row, the event list, the slot bitmaps, the bitmap of the species_a reactants' ids and the
// cursor — no particle state), and ONE 8-byte copy back that the host waits for — the event count M: the host has to learn
// the new n, also in the hook.  M = 0: the counts are added to the burner's totals and nothing else happens.  Else the host
// holds M against the products' capacities and id bounds and refuses before anything has changed (the totals included: the
// application's row is a row of its own).  Then the popcount scan of the id bitmap (fpic_renumber's kernels), the generation
// pass over the M events — it reads the reactants where they still lie —, per reactant species the compaction into the other
// particle set (count, load_scan_kernel, move), the add of the application's row to the totals, and the states: a reactant
// as remove_run leaves a species, a product as species_appended does.  The electrostatic re-deposit is inject_settle: once per
// call, and once per sub-step after the last burner that is due.
//
// The buffers of an application lie in the selection's buffer (select_buffer: it grows to the largest request and is counted
// in bytes_grid; every user of it is synchronous): the bitmap over species_a's id span, per word the marked ids below it in
// its chunk, the chunks' counts, the scan's total and the cursor, per reactant species the slot bitmap, its chunks' counts and
// their scan's total, the event list (12 bytes per possible event: min(n_a, n_b), like species n / 2).

constexpr int kBurnNow = FPIC_BURN_MAX_OPS;              // the row of the application in flight (and of fpic_burn's table)

static const fesops::Messages kBurnMessages = { FPIC_BURN_MAX_OPS, ".spec <- FPIC_BURN_MAX_OPS (4) burners are registered already", ".index <- no such registered burner" };

// a checked request into the table room of row `at`
static int burn_hold(fpic_handle* h, const fpic_burn_spec& spec, int at, BurnOp& op)
{
    OpRows& rows = h->es->diag.burn.rows;
    if (int rc = rows.room(h, fesburn::kWords, FPIC_BURN_MAX_OPS + 1, FPIC_FUSION_TABLE_MAX, true)) return rc;
    op.spec = spec;
    op.sigma.assign(spec.sigma, spec.sigma + spec.n);
    op.spec.sigma = nullptr;
    if (int rc = rows.zero(h, at)) return rc;
    HIP_TRY(h, hipMemcpyAsync(rows.table(at), op.sigma.data(), op.sigma.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the table is pageable and may change after the call)
    op.table = rows.table(at);
    return FPIC_OK;
}

static double burn_other_mass(const State* st, const fpic_burn_spec& spec) { return spec.product_b >= 0 ? st->sp[spec.product_b].mass : spec.other_mass; }

static fesburn::Rule burn_rule(const State* st, const BurnOp& op, uint32_t epoch)
{
    fpic_burn_spec s = op.spec;
    s.sigma = op.sigma.data();
    return fesburn::rule_of(s, epoch, st->W, fusion_dv(st), st->sp[s.species_a].mass, st->sp[s.species_b].mass, st->sp[s.product_a].mass, burn_other_mass(st, s));
}

// A reactant species whose survivors the move pass has written to the other particle set: the state remove_run leaves
static int burn_species_left(fpic_handle* h, Species& s, size_t kept)
{
    if (!s.thinned) s.id_span = s.n;   // (ids 0 .. n - 1 until now)
    s.thinned = true;
    s.cur ^= 1;
    s.n = kept;
    if (kept) iota3_kernel<<<blocks_for(kept), 256, 0, h->stream>>>(s.id[s.cur ^ 1], kept, 0u);
    HIP_TRY(h, hipGetLastError());
    s.ids_identity = false;
    s.binned = false;
    s.census_fresh = s.rebin_pending = s.chunk_census_fresh = false;
    s.rebin_now = false;
    s.tail_first = s.tail_count = s.n_after = 0;
    if (&s == h->es->sp.data()) h->n = kept;   // (the handle's count is its first species')
    return FPIC_OK;
}

// One application of `op` at `epoch`: the application's row into row kBurnNow, added to row `total_row` (< 0: to none);
// *events = M.  hook: a request that does not fit is a state error there.  Not settled (inject_settle is the caller's, if M).
template <typename T>
static int burn_run(fpic_handle* h, const BurnOp& op, uint32_t epoch, int total_row, bool hook, uint64_t* events)
{
    State* st = h->es;
    Diag& g = st->diag;
    const fpic_burn_spec& spec = op.spec;
    Species& sa = st->sp[spec.species_a];
    Species& sb = st->sp[spec.species_b];
    Species& s3 = st->sp[spec.product_a];
    Species* s4 = spec.product_b >= 0 ? &st->sp[spec.product_b] : nullptr;
    const bool like = spec.species_a == spec.species_b;
    const OpRows& rows = g.burn.rows;
    *events = 0;
    if (int rc = rows.zero(h, kBurnNow)) return rc;
    const fesburn::Rule r = burn_rule(st, op, epoch);
    if (!sa.n || !sb.n || !(r.f.s_max > 0)) return FPIC_OK;   // (nothing can react: nothing is launched)
    fpic_pair_spec ps{};
    ps.species_a = spec.species_a;
    ps.species_b = spec.species_b;
    if (int rc = pair_buffers(h, ps, true)) return rc;   // (an application waits for its count anyway: it may grow them)
    // the buffers: id bitmap | below | chunk counts | the scan's total, the cursor | per side: slot bitmap, chunk counts, total | the event list
    const auto pad16 = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
    const uint64_t span = id_span_of(sa);
    const size_t nwords = static_cast<size_t>((span + 31) / 32), nchunks = (nwords + kRenumberChunk - 1) / kRenumberChunk;
    const size_t below_at = pad16(nwords * sizeof(uint32_t)), chunk_at = 2 * below_at, total_at = chunk_at + pad16(nchunks * sizeof(uint32_t));
    const int sides = like ? 1 : 2;
    Species* side[2] = { &sa, &sb };
    size_t gone_at[2], counts_at[2], sum_at[2], gone_words[2], move_chunks[2], at = total_at + 16;
    for (int s = 0; s < sides; ++s) {
        gone_words[s] = (side[s]->n + 31) / 32;
        move_chunks[s] = (side[s]->n + kRemoveChunk - 1) / kRemoveChunk;
        gone_at[s] = at;
        counts_at[s] = gone_at[s] + pad16(gone_words[s] * sizeof(uint32_t));
        sum_at[s] = counts_at[s] + pad16(move_chunks[s] * sizeof(uint32_t));
        at = sum_at[s] + 16;
    }
    const size_t events_at = at;
    const size_t max_events = like ? sa.n / 2 : std::min(sa.n, sb.n);
    if (int rc = select_buffer(h, events_at + std::max<size_t>(max_events, 1) * sizeof(BurnEvent))) return rc;
    unsigned char* dev = static_cast<unsigned char*>(g.sel);
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(dev);
    uint32_t* below = reinterpret_cast<uint32_t*>(dev + below_at);
    uint32_t* chunk = reinterpret_cast<uint32_t*>(dev + chunk_at);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(dev + total_at);
    HIP_TRY(h, hipMemsetAsync(bitmap, 0, nwords * sizeof(uint32_t), h->stream));
    HIP_TRY(h, hipMemsetAsync(total, 0, 16, h->stream));
    for (int s = 0; s < sides; ++s) HIP_TRY(h, hipMemsetAsync(dev + gone_at[s], 0, gone_words[s] * sizeof(uint32_t), h->stream));
    if (int rc = pair_index<T>(h, sa, 0)) return rc;
    if (!like)
        if (int rc = pair_index<T>(h, sb, 1)) return rc;
    BurnDecideArgs<T> a{};
    const unsigned grid = pair_head(st, sa, sb, a);
    a.words = rows.row(kBurnNow);
    a.cursor = total + 1;
    a.events = reinterpret_cast<BurnEvent*>(dev + events_at);
    a.max_events = max_events;
    a.gone_a = reinterpret_cast<uint32_t*>(dev + gone_at[0]);
    a.gone_b = reinterpret_cast<uint32_t*>(dev + gone_at[like ? 0 : 1]);
    a.marked = bitmap;
    a.table = op.table;
    a.r = r;
    // (kBurnLdsBytes is below the 64 KiB a launch may ask for without an attribute: the header asserts it)
    if (like) burn_decide_kernel<T, true><<<grid, kPairThreads, kBurnLdsBytes, h->stream>>>(a);
    else burn_decide_kernel<T, false><<<grid, kPairThreads, kBurnLdsBytes, h->stream>>>(a);
    HIP_TRY(h, hipGetLastError());
    unsigned long long got = 0;
    HIP_TRY(h, hipMemcpyAsync(&got, a.cursor, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (got > max_events) return fail(h, FPIC_ERR_HIP, "fpic_burn counted %llu events among %zu and %zu particles", got, sa.n, sb.n);
    unsigned long long* const totals = total_row < 0 ? nullptr : rows.row(total_row);
    if (!got) {   // no event: the counts, and nothing else changes
        if (totals) burn_add_kernel<<<1, 1, 0, h->stream>>>(rows.row(kBurnNow), totals);
        HIP_TRY(h, hipGetLastError());
        return FPIC_OK;
    }
    const uint64_t span_3 = id_span_of(s3), span_4 = s4 ? id_span_of(*s4) : 0;
    if (const fesburn::Fit which = fesburn::fit(got, s3.n, s3.cap, span_3, s4 != nullptr, s4 ? s4->n : 0, s4 ? s4->cap : 0, span_4)) {
        const bool first = which == fesburn::kNoRoomA;
        const char* const who = fesburn::fit_field(which);
        const Species& t = first ? s3 : *s4;
        return fail(h, hook ? FPIC_ERR_STATE : FPIC_ERR_INVALID_ARG,
                    ".%s <- species %d holds %zu particles (ids below %llu) of a capacity of %zu: the %llu of this application do not fit; call fpic_reserve first; nothing was changed",
                    who, first ? spec.product_a : spec.product_b, t.n, static_cast<unsigned long long>(first ? span_3 : span_4), t.cap, got);
    }
    renumber_count_kernel<<<static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (nchunks + 3) / 4)), 256, 0, h->stream>>>(bitmap, nwords, below, chunk, nchunks);
    load_scan_kernel<<<1, 1024, 0, h->stream>>>(chunk, nchunks, total);
    BurnGenerateArgs<T> q{};
    q.slab_a = a.slab_a;
    q.slab_b = a.slab_b;
    q.n_pad_a = a.n_pad_a;
    q.n_pad_b = a.n_pad_b;
    q.events = a.events;
    q.m = static_cast<uint32_t>(got);
    q.bitmap = bitmap;
    q.below = below;
    q.offset = chunk;
    q.slab_3 = static_cast<T*>(s3.slab[s3.cur]);
    q.n_pad_3 = s3.n_pad;
    q.id_3 = s3.id[s3.cur];
    q.s0_3 = s3.n;
    q.id0_3 = static_cast<uint32_t>(span_3);
    if (s4) {
        q.slab_4 = static_cast<T*>(s4->slab[s4->cur]);
        q.n_pad_4 = s4->n_pad;
        q.id_4 = s4->id[s4->cur];
        q.s0_4 = s4->n;
        q.id0_4 = static_cast<uint32_t>(span_4);
    }
    q.words = rows.row(kBurnNow) + fesburn::kGenAt;
    q.r = r;
    const unsigned ggrid = static_cast<unsigned>(std::min<size_t>(kBurnBlocks, (static_cast<size_t>(got) + kBurnThreads - 1) / kBurnThreads));
    burn_generate_kernel<T><<<ggrid, kBurnThreads, 0, h->stream>>>(q);
    HIP_TRY(h, hipGetLastError());
    // the compaction of each reactant species into its other set
    const size_t left[2] = { like ? 2 * static_cast<size_t>(got) : static_cast<size_t>(got), static_cast<size_t>(got) };
    for (int s = 0; s < sides; ++s) {
        Species& sp = *side[s];
        BurnMoveArgs<T> m{};
        m.slab = static_cast<const T*>(sp.slab[sp.cur]);
        m.id = sp.id[sp.cur];
        m.n = sp.n;
        m.n_pad = sp.n_pad;
        m.gone = reinterpret_cast<const uint32_t*>(dev + gone_at[s]);
        m.chunk = reinterpret_cast<uint32_t*>(dev + counts_at[s]);
        m.nchunks = move_chunks[s];
        m.dst_slab = static_cast<T*>(sp.slab[sp.cur ^ 1]);
        m.dst_id = sp.id[sp.cur ^ 1];
        m.words = rows.row(kBurnNow) + fesburn::kLostAt + s * fesburn::kLostWords;
        const unsigned mgrid = static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (m.nchunks + kRemoveThreads / 64 - 1) / (kRemoveThreads / 64)));
        burn_count_kernel<<<mgrid, kRemoveThreads, 0, h->stream>>>(m.gone, m.n, m.chunk, m.nchunks);
        load_scan_kernel<<<1, 1024, 0, h->stream>>>(m.chunk, m.nchunks, reinterpret_cast<unsigned long long*>(dev + sum_at[s]));
        burn_move_kernel<T><<<mgrid, kRemoveThreads, 0, h->stream>>>(m);
        HIP_TRY(h, hipGetLastError());
    }
    if (totals) burn_add_kernel<<<1, 1, 0, h->stream>>>(rows.row(kBurnNow), totals);
    HIP_TRY(h, hipGetLastError());
    for (int s = 0; s < sides; ++s)
        if (int rc = burn_species_left(h, *side[s], side[s]->n - left[s])) return rc;
    if (int rc = species_appended(h, s3, span_3, got)) return rc;
    if (s4)
        if (int rc = species_appended(h, *s4, span_4, got)) return rc;
    *events = got;
    return FPIC_OK;
}

static int burn_apply(fpic_handle* h, const BurnOp& op, uint32_t epoch, int total_row, bool hook, uint64_t* events)
{
    return h->prec == FPIC_F32 ? burn_run<float>(h, op, epoch, total_row, hook, events) : burn_run<double>(h, op, epoch, total_row, hook, events);
}

static int burn_check(fpic_handle* h, const fpic_burn_spec* spec)
{
    State* st = h->es;
    if (const char* why = fesburn::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fesburn::check_bound(*spec, st->W, fusion_dv(st))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}

static int burn_fetch(fpic_handle* h, int row, const fpic_burn_spec& spec, fpic_burn_result* out)
{
    State* st = h->es;
    uint64_t got[fesburn::kWords] = {};
    if (int rc = st->diag.burn.rows.fetch(h, row, got)) return rc;
    const Species &sa = st->sp[spec.species_a], &sb = st->sp[spec.species_b], &s3 = st->sp[spec.product_a];
    const double mass[4] = { sa.mass, sb.mass, s3.mass, burn_other_mass(st, spec) };
    const double charge[4] = { sa.charge, sb.charge, s3.charge, spec.product_b >= 0 ? st->sp[spec.product_b].charge : 0.0 };
    fesburn::result_of(got, mass, charge, st->W, out);
    return FPIC_OK;
}

int burn(fpic_handle* h, const fpic_burn_spec* spec, fpic_burn_result* out)
{
    if (int rc = inject_refuse_decomposed(h, "fpic_burn")) return rc;
    if (int rc = burn_check(h, spec)) return rc;
    if (out) *out = fpic_burn_result{};
    BurnOp op;
    if (int rc = burn_hold(h, *spec, kBurnNow, op)) return rc;
    uint64_t events = 0;
    if (int rc = burn_apply(h, op, spec->epoch, -1, false, &events)) return rc;
    if (events)
        if (int rc = inject_settle(h)) return rc;
    if (!out) return FPIC_OK;
    if (int rc = burn_fetch(h, kBurnNow, *spec, out)) return rc;
    out->applications = 1;
    return FPIC_OK;
}

int burn_register(fpic_handle* h, const fpic_burn_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.burn;
    if (int rc = inject_refuse_decomposed(h, "fpic_burn_register")) return rc;
    if (int rc = burn_check(h, spec)) return rc;
    if (int rc = ops_check_register(h, f, kBurnMessages, every)) return rc;
    BurnOp op;
    if (int rc = burn_hold(h, *spec, static_cast<int>(f.ops.size()), op)) return rc;
    return ops_push(f, std::move(op), every, index);
}

int burn_stats(fpic_handle* h, int index, int scope, fpic_burn_result* out)
{
    auto& f = h->es->diag.burn;
    if (int rc = inject_refuse_decomposed(h, "fpic_burn_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, kBurnMessages, index, scope, out, collective)) return rc;   // (undecomposed: GLOBAL is LOCAL)
    const BurnOp& op = f.ops[index];
    *out = fpic_burn_result{};
    if (int rc = burn_fetch(h, index, op.spec, out)) return rc;
    out->applications = op.applications;
    return FPIC_OK;
}

int burn_clear(fpic_handle* h)
{
    if (int rc = inject_refuse_decomposed(h, "fpic_burn_clear")) return rc;
    return ops_clear(h->es->diag.burn);   // (every application has ended synchronised: nothing is in flight)
}

// the hook's part: every registered burner that is due, at the epoch of the sub-step, counted once it has succeeded; each
// waits for its event count.  Then ONE re-deposit and solve for all of them that had events (inject_settle).  A burner that
// fails leaves what the ones before it did, settled.
static int burn_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.burn;
    bool changed = false;
    int rc = ops_run_due<false>(f, OpsEvery{ substep }, [&](BurnOp& op, size_t k) {
        uint64_t events = 0;
        const int e = burn_apply(h, op, static_cast<uint32_t>(substep + op.spec.epoch), static_cast<int>(k), true, &events);
        if (events) changed = true;
        return e;
    });
    if (changed) {
        const std::string why = h->err;          // (the settling must not lose the message of the burner that failed)
        const int settled = inject_settle(h);
        if (rc != FPIC_OK) h->err = why;
        else rc = settled;
    }
    return rc;
}
