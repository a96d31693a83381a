// fes_pair.inc.hpp: the binary Coulomb collision operator of a CART3D handle (fpic_pair, fpic_pair_register, fpic_pair_stats,
// fpic_pair_clear) — part of fes_api.hip's translation unit (included there after fes_collide.inc.hpp, inside namespace fes).
// The rule and the checks of a request are fes_pair_core.hpp, the passes fes_pair_kernels.hpp.
//
// One application: per species of the request the cell index (count, scan, fill: three launches and one memset), then the
// pairing pass — all enqueued on the handle's stream, nothing read back.  The index buffers belong to the handle's Diag, grow
// to the largest request and are released with it; the counts go to the family's rows (fes_ops.inc.hpp), eight words per row.
// A registered operator is enqueued by the hook; fpic_pair_stats reads its row.
// A handle with a Domain is refused: between two migrations the particles of a cell can sit on two ranks, in the ghost
// planes, so a rank cannot pair a cell alone.

constexpr int kPairWords = 8;                      // per operator: pairs, strong, cells, overfull_cells, overfull_particles, (unused)
constexpr int kPairNow = FPIC_PAIR_MAX_OPS;        // the row of fpic_pair
constexpr int kPairSegLead = 4;                    // words before the first cell's: the counts are 16-byte aligned, the word before them is the zero

// TEST SWITCH (FPIC_PAIR_FORMS, read once): which form of two passes runs, for measuring one against the other
// (scripts/probe_pair.py).  Bit 0: the count privatised in LDS (pair_count_lds_kernel); bit 1: the bitonic network for
// segments above kPairRankMax; bit 2 (with bit 0): the fill privatised in LDS (pair_fill_lds_kernel).  Unset: kPairFormsDefault, what DESIGN 4.17's measurements chose.
constexpr int kPairFormsDefault = 7;
static int pair_forms()
{
    static const int forms = [] { const char* v = std::getenv("FPIC_PAIR_FORMS"); return v ? std::atoi(v) : kPairFormsDefault; }();
    return forms;
}

static size_t pair_cells(const State* st) { return static_cast<size_t>(st->nx) * st->ny * st->nz; }

static int pair_refuse_decomposed(fpic_handle* h, const char* name)
{
    if (!h->es->dom) return FPIC_OK;
    return fail(h, FPIC_ERR_STATE, "%s needs an undecomposed handle: between two migrations the particles of a cell can sit on two ranks (in the ghost planes), so a rank cannot pair a cell alone", name);
}

static int pair_room(fpic_handle* h) { return h->es->diag.pair.rows.room(h, kPairWords, FPIC_PAIR_MAX_OPS + 1); }

static int pair_grow(fpic_handle* h, uint32_t*& buf, size_t& have, size_t words)
{
    if (have >= words) return FPIC_OK;
    if (buf) { // (grows to the largest request)
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(buf));
        h->bytes_grid -= have * sizeof(uint32_t);
        buf = nullptr;
        have = 0;
    }
    if (int rc = dev_alloc(h, reinterpret_cast<void**>(&buf), words * sizeof(uint32_t), &h->bytes_grid)) return rc;
    have = words;
    return FPIC_OK;
}

// the buffers of a request: the rows and, per side, the cell words and the slots of the species' capacity
static int pair_buffers(fpic_handle* h, const fpic_pair_spec& spec, bool may_grow)
{
    State* st = h->es;
    Diag& g = st->diag;
    if (int rc = pair_room(h)) return rc;
    const int sides = spec.species_a == spec.species_b ? 1 : 2;
    for (int s = 0; s < sides; ++s) {
        const Species& sp = st->sp[s ? spec.species_b : spec.species_a];
        if (sp.n > 0xFFFFFFFFull) return fail(h, FPIC_ERR_INVALID_ARG, ".species_%c <- the cell index holds 32-bit slots", s ? 'b' : 'a');
        const size_t seg_words = pair_cells(st) + kPairSegLead, index_words = std::max<size_t>(sp.n_pad, 1);
        if (!may_grow && (g.pair_seg_words[s] < seg_words || g.pair_index_words[s] < index_words))   // (growing waits for the stream: not in the hook)
            return fail(h, FPIC_ERR_STATE, "a registered fpic_pair operator found species %d larger than at its registration: register it again", s ? spec.species_b : spec.species_a);
        if (int rc = pair_grow(h, g.pair_seg[s], g.pair_seg_words[s], seg_words)) return rc;
        if (int rc = pair_grow(h, g.pair_index[s], g.pair_index_words[s], index_words)) return rc;
    }
    return FPIC_OK;
}

// the cell index of one species into side s
template <typename T>
static int pair_index(fpic_handle* h, const Species& sp, int s)
{
    State* st = h->es;
    Diag& g = st->diag;
    HIP_TRY(h, hipMemsetAsync(g.pair_seg[s], 0, (pair_cells(st) + kPairSegLead) * sizeof(uint32_t), h->stream));
    PairIndexArgs<T> a{};
    a.slab = static_cast<const T*>(sp.slab[sp.cur]);
    a.n_pad = sp.n_pad;
    a.n = sp.n;
    a.nx = st->nx; a.ny = st->ny; a.nz = st->nz;
    a.ltx = st->ltx; a.lty = st->lty; a.ltz = st->ltz;
    a.cell = g.pair_seg[s] + kPairSegLead;
    a.index = g.pair_index[s];
    const unsigned grid = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(kPairBlocks, (sp.n + kPairThreads - 1) / kPairThreads)));
    const bool lds_count = (pair_forms() & 1) && (1u << (st->ltx + st->lty + st->ltz)) <= static_cast<unsigned>(kPairTileCellsMax);
    const unsigned turns = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(kPairBlocks, (sp.n + kPairCountTurn - 1) / kPairCountTurn)));
    if (sp.n && lds_count) pair_count_lds_kernel<T><<<turns, kPairThreads, 0, h->stream>>>(a);
    else if (sp.n) pair_count_kernel<T><<<grid, kPairThreads, 0, h->stream>>>(a);
    pair_scan_kernel<<<1, 1024, 0, h->stream>>>(a.cell, pair_cells(st));
    if (sp.n && lds_count && (pair_forms() & 4)) pair_fill_lds_kernel<T><<<turns, kPairThreads, 0, h->stream>>>(a);
    else if (sp.n) pair_fill_kernel<T><<<grid, kPairThreads, 0, h->stream>>>(a);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

// The head of the arguments of a pass that walks the cell index (pair_walk), from the two species — like species: the same
// one — and the index pair_index has left in Diag: side 0 is species a's, side 1 species b's.  Returns the grid.
template <typename S>
static unsigned pair_head(State* st, const Species& sa, const Species& sb, PairHead<S>& a)
{
    Diag& g = st->diag;
    const int side_b = &sa == &sb ? 0 : 1;
    a.slab_a = static_cast<S*>(sa.slab[sa.cur]);
    a.slab_b = static_cast<S*>(sb.slab[sb.cur]);
    a.id_a = sa.ids_identity ? nullptr : sa.id[sa.cur];
    a.id_b = sb.ids_identity ? nullptr : sb.id[sb.cur];
    a.n_pad_a = sa.n_pad;
    a.n_pad_b = sb.n_pad;
    a.seg_a = g.pair_seg[0] + kPairSegLead - 1;
    a.seg_b = g.pair_seg[side_b] + kPairSegLead - 1;
    a.index_a = g.pair_index[0];
    a.index_b = g.pair_index[side_b];
    a.ncells = static_cast<uint32_t>(pair_cells(st));
    a.rank_max = (pair_forms() & 2) ? static_cast<uint32_t>(kPairRankMax) : ~0u;
    const size_t nchunks = (pair_cells(st) + kPairChunk - 1) / kPairChunk;
    return static_cast<unsigned>(std::min<size_t>(kPairCollideBlocks, nchunks));
}

// one application at `epoch`, its counts added to words[0 .. 5): enqueued, nothing waited for
template <typename T>
static int pair_enqueue(fpic_handle* h, const fpic_pair_spec& spec, uint32_t epoch, unsigned long long* words, bool may_grow)
{
    State* st = h->es;
    if (int rc = pair_buffers(h, spec, may_grow)) return rc;
    const Species& sa = st->sp[spec.species_a];
    const Species& sb = st->sp[spec.species_b];
    const bool like = spec.species_a == spec.species_b;
    if (!sa.n || !sb.n) return FPIC_OK;   // (nothing can pair: nothing is launched)
    const double dv = (st->lx / st->nx) * (st->ly / st->ny) * (st->lz / st->nz);
    if (int rc = pair_index<T>(h, sa, 0)) return rc;
    if (!like)
        if (int rc = pair_index<T>(h, sb, 1)) return rc;
    PairArgs<T> a{};
    const unsigned grid = pair_head(st, sa, sb, a);
    a.counts = words;
    a.r = fespair::rule_of(spec, epoch, sa.mass, sa.charge, sb.mass, sb.charge, st->W, dv);
    // (kPairLdsBytes is below the 64 KiB a launch may ask for without an attribute: the header asserts it)
    if (like) pair_collide_kernel<T, true><<<grid, kPairThreads, kPairLdsBytes, h->stream>>>(a);
    else pair_collide_kernel<T, false><<<grid, kPairThreads, kPairLdsBytes, h->stream>>>(a);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

static int pair_apply(fpic_handle* h, const fpic_pair_spec& spec, uint32_t epoch, unsigned long long* words, bool may_grow)
{
    return h->prec == FPIC_F32 ? pair_enqueue<float>(h, spec, epoch, words, may_grow) : pair_enqueue<double>(h, spec, epoch, words, may_grow);
}

static void pair_result(fpic_pair_result* out, uint64_t applications, const uint64_t* got)
{
    out->applications = applications;
    out->pairs = got[0];
    out->strong = got[1];
    out->cells = got[2];
    out->overfull_cells = got[3];
    out->overfull_particles = got[4];
}

int pair(fpic_handle* h, const fpic_pair_spec* spec, fpic_pair_result* out)
{
    State* st = h->es;
    const OpRows& rows = st->diag.pair.rows;
    if (int rc = pair_refuse_decomposed(h, "fpic_pair")) return rc;
    if (const char* why = fespair::check(spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (out) *out = fpic_pair_result{};
    if (int rc = pair_room(h)) return rc;
    if (int rc = rows.zero(h, kPairNow)) return rc;
    if (int rc = pair_apply(h, *spec, spec->epoch, rows.row(kPairNow), true)) return rc;
    uint64_t got[kPairWords] = {};
    if (int rc = rows.fetch(h, kPairNow, got)) return rc;
    if (out) pair_result(out, 1, got);
    return FPIC_OK;
}

int pair_register(fpic_handle* h, const fpic_pair_spec* spec, int every, int* index)
{
    auto& f = h->es->diag.pair;
    if (int rc = pair_refuse_decomposed(h, "fpic_pair_register")) return rc;
    if (const char* why = fespair::check(spec, static_cast<int>(h->es->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (int rc = ops_check_register(h, f, fesops::kPair, every)) return rc;
    if (int rc = pair_buffers(h, *spec, true)) return rc;   // (sized now: the hook finds them in place and never grows them)
    if (int rc = f.rows.zero(h, f.ops.size())) return rc;
    PairOp op;
    op.spec = *spec;
    return ops_push(f, op, every, index);
}

int pair_stats(fpic_handle* h, int index, int scope, fpic_pair_result* out)
{
    auto& f = h->es->diag.pair;
    if (int rc = pair_refuse_decomposed(h, "fpic_pair_stats")) return rc;
    bool collective = false;
    if (int rc = ops_stats_head(h, f, fesops::kPair, index, scope, out, collective)) return rc;
    uint64_t got[kPairWords] = {};
    if (int rc = f.rows.fetch(h, index, got)) return rc;
    if (collective)
        if (int rc = diag_sum_ranks(h, got, kPairWords)) return rc;
    pair_result(out, f.ops[index].applications, got);
    return FPIC_OK;
}

int pair_clear(fpic_handle* h)
{
    if (int rc = pair_refuse_decomposed(h, "fpic_pair_clear")) return rc;
    return ops_clear(h->es->diag.pair);
}

// the hook's part: every registered operator that is due, at the epoch of the sub-step; the cell index does not grow here
static int pair_after_substep(fpic_handle* h, uint64_t substep)
{
    auto& f = h->es->diag.pair;
    return ops_run_due<true>(f, OpsEvery{ substep }, [&](PairOp& op, size_t k) { return pair_apply(h, op.spec, static_cast<uint32_t>(substep + op.spec.epoch), f.rows.row(k), false); });
}
