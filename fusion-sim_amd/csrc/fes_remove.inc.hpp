// fes_remove.inc.hpp: the absorbing particle sinks of a CART3D handle (fpic_remove, fpic_remove_register, fpic_remove_stats,
// fpic_remove_clear, fpic_renumber) — part of fes_api.hip's translation unit (included there after
// fes_fusion_spectrum.inc.hpp, inside namespace fes).  The rule and the checks of a request are fes_remove_core.hpp, the
// passes fes_remove_kernels.hpp.
//
// One application: the mark pass over the slots [0, n) (the chunks' survivor counts and the removed count into the
// selection's buffer, which grows to the largest request), and ONE 8-byte copy back that the host waits for — the removed
// count: the host has to learn the new n, also when the application is a registered one in the hook.  Nothing removed:
// nothing else happens; no scan is launched, no buffer swapped, no flag, field or bin table touched.  Else the scan of the
// counts (load_scan_kernel), the move pass into the other particle set (which tallies what left into the workgroups' partial
// rows), the combining launch (this application's row, added to the operator's totals), the swap, and the state load_keep
// and fpic_domain_set_particles leave: n lowered, the live set holding the survivors with their ids, the other set's ids the
// slot numbers, nothing binned, no census; the species is THINNED.  An electrostatic handle whose fields were ready deposits
// and solves again here (the tail of precalc()), so that the next sub-step gathers the field of the survivors; a full-EM
// handle keeps E, B and its readiness as they are.

// the family's rows (fes_ops.inc.hpp), kDiagWords words each: the operators' totals, the row of the last application (the
// call's row), behind it a row whose first word is the mark pass's counter, then the move pass's partial rows
constexpr int kRemoveLast = FPIC_REMOVE_MAX_OPS;
constexpr int kRemoveGone = kRemoveLast + 1, kRemovePartial = kRemoveLast + 2;

static int remove_refuse_decomposed(fpic_handle* h, const char* name)
{
    if (!h->es->dom) return FPIC_OK;
    return fail(h, FPIC_ERR_STATE, "%s needs an undecomposed handle: a rank's dead slots and the arrivals of a migration that rides on its next push would need a protocol of their own to compact", name);
}

static int remove_room(fpic_handle* h) { return h->es->diag.remove.rows.room(h, kDiagWords, static_cast<size_t>(kRemovePartial) + kRemoveBlocks); }

template <typename T, int NA>
static void remove_launch(fpic_handle* h, const RemoveArgs<T>& a, unsigned grid, bool move)
{
    if (move) remove_move_kernel<T, NA><<<grid, kRemoveThreads, 0, h->stream>>>(a);
    else remove_mark_kernel<T, NA><<<grid, kRemoveThreads, 0, h->stream>>>(a);
}
template <typename T>
static void remove_launch_na(fpic_handle* h, const RemoveArgs<T>& a, int na, unsigned grid, bool move)
{
    switch (na) {
    case 0: remove_launch<T, 0>(h, a, grid, move); break;
    case 1: remove_launch<T, 1>(h, a, grid, move); break;
    case 2: remove_launch<T, 2>(h, a, grid, move); break;
    case 3: remove_launch<T, 3>(h, a, grid, move); break;
    case 4: remove_launch<T, 4>(h, a, grid, move); break;
    case 5: remove_launch<T, 5>(h, a, grid, move); break;
    default: remove_launch<T, 6>(h, a, grid, move); break;
    }
}

// one application of a checked request: this application's row into row kRemoveLast, added to row `total_row` (< 0: to none);
// *removed = what left.  Synchronised.
template <typename T>
static int remove_run(fpic_handle* h, const fpic_remove_spec& spec, int total_row, uint64_t* scanned, uint64_t* removed)
{
    State* st = h->es;
    Diag& g = st->diag;
    Species& s = st->sp[spec.species];
    *scanned = s.n;
    *removed = 0;
    if (int rc = remove_room(h)) return rc;
    const OpRows& rows = g.remove.rows;
    unsigned long long* gone = rows.row(kRemoveGone);
    if (int rc = rows.zero(h, kRemoveLast, 2)) return rc;   // (the last application's row and the counter's behind it)
    if (!s.n || fesrem::never(spec)) return FPIC_OK;   // (nothing can leave: nothing is launched)
    const size_t n = s.n, nchunks = (n + kRemoveChunk - 1) / kRemoveChunk;
    // the chunks' counts, then 8 bytes for the scan's total (the selection's buffer, as load_keep)
    const size_t total_at = (nchunks * sizeof(uint32_t) + 15) / 16 * 16;
    if (int rc = select_buffer(h, total_at + 16)) return rc;
    unsigned char* dev = static_cast<unsigned char*>(g.sel);
    RemoveArgs<T> a{};
    a.slab = static_cast<const T*>(s.slab[s.cur]);
    a.id = s.id[s.cur];
    a.n = n;
    a.n_pad = s.n_pad;
    // the arrays the passes stream, in slab order: those the terms name (select_local's layout)
    const fpic_select_spec sel = fesrem::select_of(spec);
    const uint32_t arrays = fessel::arrays_of(sel);
    int na = 0, at[6] = {};
    for (int c = 0; c < 6; ++c)
        if (arrays >> c & 1u) {
            at[c] = na;
            a.src[na++] = a.slab + c * s.n_pad;
        }
    for (int t = 0; t < spec.nterms; ++t) {
        if (spec.axis[t] == FPIC_AXIS_V2) {
            a.v2 = 1;
            a.v2_lo = spec.lo[t];
            a.v2_hi = spec.hi[t];
        } else {
            const int k = at[spec.axis[t]];
            a.term |= 1u << k;
            a.lo[k] = spec.lo[t];
            a.hi[k] = spec.hi[t];
        }
    }
    a.id_mod = spec.id_mod;
    a.id_rem = spec.id_rem;
    a.flags = spec.flags;
    a.chunk = reinterpret_cast<uint32_t*>(dev);
    a.nchunks = nchunks;
    a.gone = gone;
    a.partial = rows.row(kRemovePartial);
    a.dst_slab = static_cast<T*>(s.slab[s.cur ^ 1]);
    a.dst_id = s.id[s.cur ^ 1];
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (nchunks + kRemoveThreads / 64 - 1) / (kRemoveThreads / 64)));
    remove_launch_na<T>(h, a, na, grid, false);
    HIP_TRY(h, hipGetLastError());
    unsigned long long got = 0;
    HIP_TRY(h, hipMemcpyAsync(&got, gone, sizeof(got), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!got) return FPIC_OK;   // nothing left: nothing changes
    if (got > n) return fail(h, FPIC_ERR_HIP, "fpic_remove counted %llu removed particles of %zu", got, n);
    *removed = got;
    const size_t kept = n - static_cast<size_t>(got);
    // (everything removed: the move pass still runs, for the tally; it writes no survivor)
    load_scan_kernel<<<1, 1024, 0, h->stream>>>(a.chunk, nchunks, reinterpret_cast<unsigned long long*>(dev + total_at));
    remove_launch_na<T>(h, a, na, grid, true);
    remove_combine_kernel<<<1, kDiagThreads, 0, h->stream>>>(a.partial, static_cast<int>(grid), rows.row(kRemoveLast), total_row < 0 ? nullptr : rows.row(total_row));
    HIP_TRY(h, hipGetLastError());
    // the state load_keep and fpic_domain_set_particles leave: the live set holds the particles in slot order with their
    // ids, the other set's ids are the slot numbers (the next binning writes both anew)
    if (!s.thinned) s.id_span = n;   // (ids 0 .. n - 1 until now)
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
    if (&s == st->sp.data()) h->n = kept;   // (the handle's count is its first species')
    // the electrostatic cycle gathers E of the last solve at the start of the next sub-step: that field still holds the
    // removed charge.  The tail of precalc(): bin where it would, deposit the survivors, solve.
    if (st->solver == FPIC_SOLVER_POISSON_FFT && st->fields_ready)
        if (int rc = precalc(h)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

static int remove_apply(fpic_handle* h, const fpic_remove_spec& spec, int total_row, uint64_t* scanned, uint64_t* removed)
{
    return h->prec == FPIC_F32 ? remove_run<float>(h, spec, total_row, scanned, removed) : remove_run<double>(h, spec, total_row, scanned, removed);
}

static int remove_fetch(fpic_handle* h, int row, const Species& sp, fpic_remove_result* out)
{
    State* st = h->es;
    uint64_t got[kDiagWords] = {};
    if (int rc = st->diag.remove.rows.fetch(h, row, got)) return rc;
    fesrem::result_of(got, sp.mass, sp.charge, st->W, out);
    return FPIC_OK;
}

int remove(fpic_handle* h, const fpic_remove_spec* spec, fpic_remove_result* out)
{
    State* st = h->es;
    if (int rc = remove_refuse_decomposed(h, "fpic_remove")) return rc;
    if (const char* why = fesrem::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_remove_result{};
    uint64_t scanned = 0, removed = 0;
    if (int rc = remove_apply(h, *spec, -1, &scanned, &removed)) return rc;
    if (!out) return FPIC_OK;
    if (int rc = remove_fetch(h, kRemoveLast, st->sp[spec->species], out)) return rc;
    out->applications = 1;
    out->scanned = scanned;
    return FPIC_OK;
}

int remove_register(fpic_handle* h, const fpic_remove_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.remove;
    if (int rc = remove_refuse_decomposed(h, "fpic_remove_register")) return rc;
    if (const char* why = fesrem::check(spec, static_cast<int>(h->es->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, fesops::kRemove, every)) return rc;
    if (int rc = remove_room(h)) return rc;
    if (int rc = f.rows.zero(h, f.ops.size())) return rc;
    RemoveOp op;
    op.spec = *spec;
    return ops_push(f, op, every, index);
}

int remove_stats(fpic_handle* h, int index, int scope, fpic_remove_result* out)
{
    State* st = h->es;
    auto& f = st->diag.remove;
    if (int rc = remove_refuse_decomposed(h, "fpic_remove_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kRemove, index, scope, out, collective)) return rc;   // (undecomposed: GLOBAL is LOCAL)
    const RemoveOp& op = f.ops[index];
    *out = fpic_remove_result{};
    if (int rc = remove_fetch(h, index, st->sp[op.spec.species], out)) return rc;
    out->applications = op.applications;
    out->scanned = op.scanned;
    return FPIC_OK;
}

int remove_clear(fpic_handle* h)
{
    if (int rc = remove_refuse_decomposed(h, "fpic_remove_clear")) return rc;
    return ops_clear(h->es->diag.remove);   // (every application has ended synchronised: nothing is in flight)
}

// the hook's part: every registered sink that is due; an application is counted once it has succeeded.  Each waits for its
// removed count
static int remove_after_substep(fpic_handle* h, uint64_t substep)
{
    return ops_run_due<false>(h->es->diag.remove, OpsEvery{ substep }, [&](RemoveOp& op, size_t k) {
        uint64_t scanned = 0, removed = 0;
        if (int rc = remove_apply(h, op.spec, static_cast<int>(k), &scanned, &removed)) return rc;
        op.scanned += scanned;
        return static_cast<int>(FPIC_OK);
    });
}

int renumber(fpic_handle* h, int species, uint64_t* n_out)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = remove_refuse_decomposed(h, "fpic_renumber")) return rc;
    if (int rc = check_species(h, species)) return rc;
    Species& s = st->sp[species];
    if (n_out) *n_out = s.n;
    if (!s.thinned) return FPIC_OK;
    if (g.rec[kRecSeries].every)
        return fail(h, FPIC_ERR_STATE, "fpic_renumber while a series is being recorded: its tracers are named by id, and the ids are about to change; stop the recording first");
    if (ops_registered(g))
        return fail(h, FPIC_ERR_STATE, "fpic_renumber while an operator is registered: registered operators draw per-id random words or thin by id, and the ids are about to change; clear the registrations first");
    const size_t n = s.n;
    if (n) {
        const size_t nwords = static_cast<size_t>((s.id_span + 31) / 32), nchunks = (nwords + kRenumberChunk - 1) / kRenumberChunk;
        // the bitmap, per word the live ids below it in its chunk, the chunks' counts, 8 bytes for the total
        const size_t below_at = (nwords * sizeof(uint32_t) + 15) / 16 * 16, chunk_at = 2 * below_at, total_at = chunk_at + (nchunks * sizeof(uint32_t) + 15) / 16 * 16;
        if (int rc = select_buffer(h, total_at + 16)) return rc;
        unsigned char* dev = static_cast<unsigned char*>(g.sel);
        uint32_t* bitmap = reinterpret_cast<uint32_t*>(dev);
        uint32_t* below = reinterpret_cast<uint32_t*>(dev + below_at);
        uint32_t* chunk = reinterpret_cast<uint32_t*>(dev + chunk_at);
        unsigned long long* total = reinterpret_cast<unsigned long long*>(dev + total_at);
        HIP_TRY(h, hipMemsetAsync(bitmap, 0, nwords * sizeof(uint32_t), h->stream));
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (n + 255) / 256));
        renumber_mark_kernel<<<grid, 256, 0, h->stream>>>(s.id[s.cur], n, bitmap);
        renumber_count_kernel<<<static_cast<unsigned>(std::min<size_t>(kRemoveBlocks, (nchunks + 3) / 4)), 256, 0, h->stream>>>(bitmap, nwords, below, chunk, nchunks);
        load_scan_kernel<<<1, 1024, 0, h->stream>>>(chunk, nchunks, total);
        renumber_assign_kernel<<<grid, 256, 0, h->stream>>>(s.id[s.cur], n, bitmap, below, chunk);
        HIP_TRY(h, hipGetLastError());
        unsigned long long got = 0;
        HIP_TRY(h, hipMemcpyAsync(&got, total, sizeof(got), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (got != n) return fail(h, FPIC_ERR_STATE, "fpic_renumber found %llu distinct ids among %zu particles", got, n);
    }
    s.thinned = false;
    s.id_span = 0;
    return FPIC_OK;
}
