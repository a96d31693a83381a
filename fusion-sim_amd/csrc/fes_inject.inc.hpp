// fes_inject.inc.hpp: the particle sources of a CART3D handle (fpic_reserve, fpic_population, fpic_inject,
// fpic_inject_register, fpic_inject_stats, fpic_inject_clear) — part of fes_api.hip's translation unit (included there after
// fes_remove.inc.hpp, inside namespace fes).  The rule and the checks of a request are fes_inject_core.hpp, the pass
// fes_inject_kernels.hpp.
//
// One application: the host knows everything in advance — the sequence numbers (first + k count + l), the slots [n, n + count),
// the ids (id span + l) — and holds them against 2^32 and the capacity before anything is touched.  Then ONE generation launch
// into the live set (which tallies what the species gained into the workgroups' partial rows), the combining launch (this
// application's row, added to the source's totals), and the state load_keep with FPIC_LOAD_APPEND leaves: n raised, the
// other set's ids the slot numbers, nothing binned, no census.  Nothing is read back.  An electrostatic handle whose fields
// were ready deposits and solves again (the tail of precalc()), so that the next sub-step gathers the field of the grown
// population — once per call, and once per sub-step for all the registered sources due on it; a full-EM handle keeps E, B
// and its readiness as they are.
//
// fpic_reserve: new arrays of the larger stride, initialised as alloc_species initialises them, the live set copied column by
// column with its ids, the tables sized by the capacity (the work lists, the per-item census) allocated anew, the old ones
// freed.  Who else reads cap, n_pad or work_cap: the joint work list sizes itself from the species' cap at every launch and
// regrows (ensure_joint_list; its signature is cleared here), EmPushArgs in Species::em_args are stored anew by every
// full-EM launch, the kernels' arguments are formed per launch from the Species, the cell index of the binary operators
// (fpic_pair, fpic_fusion, fpic_fusion_spectrum) is sized from n_pad when one is registered and regrown by reserve() itself,
// and the message buffers of a decomposition (fpic_domain_init) are sized when it is made — after which fpic_reserve is refused.

// the family's rows (fes_ops.inc.hpp), kDiagWords words each: the sources' totals, the row of the last application (the call's
// row), behind it the generation pass's partial rows
constexpr int kInjectLast = FPIC_INJECT_MAX_OPS;
constexpr int kInjectPartial = kInjectLast + 1;

static int inject_refuse_decomposed(fpic_handle* h, const char* name)
{
    if (!h->es->dom) return FPIC_OK;
    return fail(h, FPIC_ERR_STATE, "%s needs an undecomposed handle: a rank's arrivals ride on its next push, and its message buffers were sized from the capacity it had", name);
}

static int inject_room(fpic_handle* h) { return h->es->diag.inject.rows.room(h, kDiagWords, static_cast<size_t>(kInjectPartial) + kInjectBlocks); }

// what follows the applications of a call or of a sub-step.  The electrostatic cycle gathers E of the last solve at the start
// of the next sub-step: that field lacks the new charge.  The tail of precalc(): bin where it would, deposit the grown
// population, solve.  Then the host waits once.
static int inject_settle(fpic_handle* h)
{
    State* st = h->es;
    if (st->solver == FPIC_SOLVER_POISSON_FFT && st->fields_ready)
        if (int rc = precalc(h)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

// A species whose live set has just gained `count` particles in the slots [n, n + count) with the ids span + l (a source's
// generation pass, an ioniser's): the state load_keep leaves after an append — the live set holds the particles in slot order
// with their ids, the other set's ids are the slot numbers (the next binning writes both anew), nothing binned, no census
static int species_appended(fpic_handle* h, Species& s, uint64_t span, uint64_t count)
{
    if (s.thinned) s.id_span = span + count;   // (not thinned: the ids stay 0 .. n - 1, id_span_of() follows n)
    s.n += static_cast<size_t>(count);
    iota3_kernel<<<blocks_for(s.n), 256, 0, h->stream>>>(s.id[s.cur ^ 1], s.n, 0u);
    HIP_TRY(h, hipGetLastError());
    s.binned = false;
    s.census_fresh = s.rebin_pending = s.chunk_census_fresh = false;
    s.rebin_now = false;
    s.tail_first = s.tail_count = s.n_after = 0;
    if (&s == h->es->sp.data()) h->n = s.n;   // (the handle's count is its first species')
    return FPIC_OK;
}

// application k (counted from the epoch on) of a checked request: this application's row into row kInjectLast, added to row
// `total_row` (< 0: to none).  hook: called from the sub-step hook — a request that does not fit is a state error there, and the
// re-deposit and the wait are the hook's, once (inject_settle); otherwise the call ends settled.  count = 0: nothing is launched,
// nothing changes.
template <typename T>
static int inject_run(fpic_handle* h, const fpic_inject_spec& spec, uint64_t k, int total_row, bool hook)
{
    State* st = h->es;
    Diag& g = st->diag;
    Species& s = st->sp[spec.load.species];
    const uint64_t count = spec.load.count;
    if (!count) return FPIC_OK;
    uint64_t first = 0;
    if (!fesinj::first_of(spec, k, &first))
        return fail(h, FPIC_ERR_STATE, "fpic_inject: application %llu of the source would pass the sequence numbers' bound, first + count <= 2^32 - 1 (first %llu, count %llu, epoch %llu); nothing was changed",
                    static_cast<unsigned long long>(k), static_cast<unsigned long long>(spec.load.first), static_cast<unsigned long long>(count),
                    static_cast<unsigned long long>(spec.epoch));
    const uint64_t span = id_span_of(s);
    if (!fesinj::fits(s.n, s.cap, span, count))
        return fail(h, hook ? FPIC_ERR_STATE : FPIC_ERR_INVALID_ARG,
                    ".count <- species %d holds %zu particles (ids below %llu) of a capacity of %zu: %llu more do not fit; call fpic_reserve first; nothing was changed",
                    spec.load.species, s.n, static_cast<unsigned long long>(span), s.cap, static_cast<unsigned long long>(count));
    if (int rc = inject_room(h)) return rc;
    const OpRows& rows = g.inject.rows;
    const double L[3] = { st->lx, st->ly, st->lz };
    InjectArgs<T> a{};
    a.slab = static_cast<T*>(s.slab[s.cur]);
    a.id = s.id[s.cur];
    a.n_pad = s.n_pad;
    a.s0 = s.n;
    a.s1 = s.n + static_cast<size_t>(count);
    a.first = static_cast<uint32_t>(first);
    a.id0 = static_cast<uint32_t>(span);
    a.partial = rows.row(kInjectPartial);
    a.q = fesinj::rule_of(spec, first, L, h->spec.dt);
    const size_t groups = (a.s1 + kInjectGroup - 1) / kInjectGroup - a.s0 / kInjectGroup;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(kInjectBlocks, (groups + kInjectThreads - 1) / kInjectThreads));
    if (spec.kind == FPIC_INJECT_FLUX) inject_kernel<T, true><<<grid, kInjectThreads, 0, h->stream>>>(a);
    else inject_kernel<T, false><<<grid, kInjectThreads, 0, h->stream>>>(a);
    remove_combine_kernel<<<1, kDiagThreads, 0, h->stream>>>(a.partial, static_cast<int>(grid), rows.row(kInjectLast), total_row < 0 ? nullptr : rows.row(total_row));
    HIP_TRY(h, hipGetLastError());
    if (int rc = species_appended(h, s, span, count)) return rc;
    return hook ? FPIC_OK : inject_settle(h);   // (the hook settles once, after the last source that is due)
}

static int inject_apply(fpic_handle* h, const fpic_inject_spec& spec, uint64_t k, int total_row, bool hook)
{
    return h->prec == FPIC_F32 ? inject_run<float>(h, spec, k, total_row, hook) : inject_run<double>(h, spec, k, total_row, hook);
}

static int inject_check(fpic_handle* h, const fpic_inject_spec* spec)
{
    const State* st = h->es;
    const double L[3] = { st->lx, st->ly, st->lz };
    if (const char* why = fesinj::check(spec, static_cast<int>(st->sp.size()), L)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    return FPIC_OK;
}

static int inject_fetch(fpic_handle* h, int row, const Species& sp, fpic_inject_result* out)
{
    State* st = h->es;
    uint64_t got[kDiagWords] = {};
    if (int rc = st->diag.inject.rows.fetch(h, row, got)) return rc;
    fesinj::result_of(got, sp.mass, sp.charge, st->W, out);
    return FPIC_OK;
}

int inject(fpic_handle* h, const fpic_inject_spec* spec, fpic_inject_result* out)
{
    State* st = h->es;
    if (int rc = inject_refuse_decomposed(h, "fpic_inject")) return rc;
    if (int rc = inject_check(h, spec)) return rc;
    if (out) *out = fpic_inject_result{};
    if (!spec->load.count) return FPIC_OK;
    if (int rc = inject_apply(h, *spec, 0, -1, false)) return rc;
    if (!out) return FPIC_OK;
    if (int rc = inject_fetch(h, kInjectLast, st->sp[spec->load.species], out)) return rc;
    out->applications = 1;
    return FPIC_OK;
}

int inject_register(fpic_handle* h, const fpic_inject_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.inject;
    if (int rc = inject_refuse_decomposed(h, "fpic_inject_register")) return rc;
    if (int rc = inject_check(h, spec)) return rc;
    if (int rc = ops_check_register(h, f, fesops::kInject, every)) return rc;
    if (int rc = inject_room(h)) return rc;
    if (int rc = f.rows.zero(h, f.ops.size())) return rc;
    InjectOp op;
    op.spec = *spec;
    return ops_push(f, op, every, index);
}

int inject_stats(fpic_handle* h, int index, int scope, fpic_inject_result* out)
{
    State* st = h->es;
    auto& f = st->diag.inject;
    if (int rc = inject_refuse_decomposed(h, "fpic_inject_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kInject, index, scope, out, collective)) return rc;   // (undecomposed: GLOBAL is LOCAL)
    const InjectOp& op = f.ops[index];
    *out = fpic_inject_result{};
    if (int rc = inject_fetch(h, index, st->sp[op.spec.load.species], out)) return rc;
    out->applications = op.applications;
    return FPIC_OK;
}

int inject_clear(fpic_handle* h)
{
    if (int rc = inject_refuse_decomposed(h, "fpic_inject_clear")) return rc;
    return ops_clear(h->es->diag.inject);   // (every application has ended synchronised: nothing is in flight)
}

// the hook's part: every registered source that is due — a source of count 0 never is —, its applications so far the
// application number, counted once it has succeeded; their launches queued one behind the other, then ONE re-deposit and solve
// for all of them and one wait (the charge grid is a function of the positions: the result is that of settling after each).
// A source that fails leaves what the ones before it did, settled.
static int inject_after_substep(fpic_handle* h, uint64_t substep)
{
    bool applied = false;
    int rc = ops_run_due<false>(h->es->diag.inject, [&](const InjectOp& op) { return OpsEvery{ substep }(op) && op.spec.load.count != 0; },
                                [&](InjectOp& op, size_t k) {
                                    const int e = inject_apply(h, op.spec, op.applications, static_cast<int>(k), true);
                                    if (e == FPIC_OK) applied = true;
                                    return e;
                                });
    if (applied) {
        const std::string why = h->err;          // (the settling must not lose the message of the source that failed)
        const int settled = inject_settle(h);
        if (rc != FPIC_OK) h->err = why;
        else rc = settled;
    }
    return rc;
}

int population(fpic_handle* h, int species, uint64_t* n, uint64_t* capacity, uint64_t* id_span)
{
    if (int rc = check_species(h, species)) return rc;
    const Species& s = h->es->sp[species];
    if (n) *n = s.n;
    if (capacity) *capacity = s.cap;
    if (id_span) *id_span = id_span_of(s);
    return FPIC_OK;
}

template <typename T>
static int reserve_run(fpic_handle* h, Species& s, size_t capacity)
{
    State* st = h->es;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Species old = s;   // (the pointers: freed below, or put back if an allocation fails)
    const uint64_t particles_before = h->bytes_particles, grid_before = h->bytes_grid;
    const size_t old_set = old.n_pad * (6 * sizeof(T) + sizeof(uint32_t));
    const size_t old_tables = (sizeof(uint32_t) * kNbr3 * old.chunk_census_items) + 2 * sizeof(BlockWork) * old.work_cap;
    s.cap = capacity;
    s.n_pad = (s.cap + 1023) / 1024 * 1024;
    s.work_cap = (s.cap + kChunk3 - 1) / kChunk3 + st->ntiles;
    s.chunk_census_items = s.work_cap;
    s.slab[0] = s.slab[1] = nullptr;
    s.id[0] = s.id[1] = nullptr;
    s.chunk_census = nullptr;
    s.work2[0] = s.work2[1] = nullptr;
    int rc = FPIC_OK;
    for (int k = 0; k < 2 && !rc; ++k) {
        if ((rc = dev_alloc(h, &s.slab[k], 6 * s.n_pad * sizeof(T), &h->bytes_particles))) break;
        if ((rc = dev_alloc(h, reinterpret_cast<void**>(&s.id[k]), s.n_pad * sizeof(uint32_t), &h->bytes_particles))) break;
        rc = dev_alloc(h, reinterpret_cast<void**>(&s.work2[k]), sizeof(BlockWork) * s.work_cap, &h->bytes_grid);
    }
    if (!rc) rc = dev_alloc(h, reinterpret_cast<void**>(&s.chunk_census), sizeof(uint32_t) * kNbr3 * s.work_cap, &h->bytes_grid);
    if (rc) {   // nothing has been touched: the species keeps its arrays
        for (void* p : { s.slab[0], s.slab[1], static_cast<void*>(s.id[0]), static_cast<void*>(s.id[1]), static_cast<void*>(s.work2[0]), static_cast<void*>(s.work2[1]),
                         static_cast<void*>(s.chunk_census) })
            if (p) (void)hipFree(p);
        s = old;
        h->bytes_particles = particles_before;
        h->bytes_grid = grid_before;
        return rc;
    }
    for (int k = 0; k < 2; ++k) init3_kernel<T><<<blocks_for(s.n_pad), 256, 0, h->stream>>>(static_cast<T*>(s.slab[k]), s.n_pad, s.id[k]);
    if (s.n)
        reserve_copy_kernel<T><<<blocks_for(s.n), 256, 0, h->stream>>>(static_cast<const T*>(old.slab[old.cur]), old.n_pad, old.id[old.cur], static_cast<T*>(s.slab[s.cur]), s.n_pad,
                                                                    s.id[s.cur], s.n);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (void* p : { old.slab[0], old.slab[1], static_cast<void*>(old.id[0]), static_cast<void*>(old.id[1]), static_cast<void*>(old.work2[0]), static_cast<void*>(old.work2[1]),
                     static_cast<void*>(old.chunk_census) })
        if (p) (void)hipFree(p);
    h->bytes_particles -= 2 * old_set;
    h->bytes_grid -= old_tables;
    // as after an upload: the live set is in place, nothing is binned; n, the ids' form, the mark of a thinned species, the
    // fields and their readiness stay (no position moved)
    s.binned = false;
    s.census_fresh = s.rebin_pending = s.chunk_census_fresh = false;
    s.rebin_now = false;
    s.tail_first = s.tail_count = s.n_after = 0;
    s.layout++;
    st->joint_built_from.clear();   // (the joint list regrows from the species' cap at its next launch)
    return FPIC_OK;
}

int reserve(fpic_handle* h, int species, uint64_t capacity, uint64_t* capacity_out)
{
    State* st = h->es;
    if (int rc = inject_refuse_decomposed(h, "fpic_reserve")) return rc;
    if (int rc = check_species(h, species)) return rc;
    Species& s = st->sp[species];
    if (capacity > s.cap) {
        if (const char* why = fesinj::check_capacity(capacity)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
        // the cell index of the binary operators (fes_pair.inc.hpp; the fusion tallies and spectra share it) holds one slot word
        // per padded particle and is sized when an operator is registered: the hook never grows it (growing waits for the
        // stream) and refuses a species it finds larger.  This call is synchronous, so the index buffers that exist follow the
        // new stride here, and an operator registered before the reserve finds them large enough at its next application.
        // They grow FIRST, and each new buffer is allocated before the old one is freed: an allocation that fails leaves the
        // species, the index and every registered operator with what they had (a buffer that has already grown stays larger
        // than it need be, which nobody reads).  Both sides follow whichever species grows — a side serves species a or b of
        // any request, so the side that never indexes this species is over-allocated by 4 bytes per slot, knowingly
        Diag& g = st->diag;
        const size_t n_pad = (static_cast<size_t>(capacity) + 1023) / 1024 * 1024;   // (reserve_run's stride)
        for (int k = 0; k < 2; ++k) {
            if (!g.pair_index[k] || g.pair_index_words[k] >= n_pad) continue;
            void* fresh = nullptr;
            if (int rc = dev_alloc(h, &fresh, n_pad * sizeof(uint32_t), &h->bytes_grid)) return rc;
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, hipFree(g.pair_index[k]));
            h->bytes_grid -= g.pair_index_words[k] * sizeof(uint32_t);
            g.pair_index[k] = static_cast<uint32_t*>(fresh);
            g.pair_index_words[k] = n_pad;
        }
        if (int rc = h->prec == FPIC_F32 ? reserve_run<float>(h, s, static_cast<size_t>(capacity)) : reserve_run<double>(h, s, static_cast<size_t>(capacity))) return rc;
    }
    if (capacity_out) *capacity_out = s.cap;
    return FPIC_OK;
}
