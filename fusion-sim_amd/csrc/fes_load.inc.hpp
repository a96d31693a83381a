// fes_load.inc.hpp: the particle loader of a CART3D handle (fpic_load) — part of fes_api.hip's translation unit (included
// there after fes_select.inc.hpp, inside namespace fes).  The rule and the checks of a request are fes_load_core.hpp, the
// passes fes_load_kernels.hpp.
//
// An undecomposed handle: one launch of load_slots_kernel over the slots that can hold the range (the range itself while
// the species is in the caller's order, every slot once it has been binned), then what set_particles sets after an upload.
// A rank of a decomposition: the counting pass of load_keep_kernel over the indices, the scan of the chunks' counts, the
// total copied back and held against the capacity — nothing has been touched until here —, then the writing pass and the
// state domain_set_particles leaves: slot order = ascending id, the ids beside the particles.
// A profiled load (fpic_load_profile) takes the same two routes with the instances of the kernels that read the tables; the
// tables are laid out on the host (fesload::layout: a density table beside its cumulative masses) and uploaded per call into
// Diag::load_tab.  Without a table the call is fpic_load's: the same instances, no buffer.
// A radial load (fpic_load_radial, the rule fes_load_radial_core.hpp) is the third set of instances on the same two routes;
// its one block of tables (fesload::radial_layout) goes through the same buffer and is staged whole in the LDS.

template <typename T, bool POS, bool VEL, typename Args>
static void load_slots_launch(fpic_handle* h, const Args& a)
{
    const size_t groups = (a.s1 + 3) / 4 - a.s0 / 4;
    const unsigned grid = static_cast<unsigned>(std::min<size_t>(kLoadBlocks, (groups + kLoadThreads - 1) / kLoadThreads));
    size_t lds = 0;   // the searched tables of a profiled load (stage_tables); at most kLoadLdsBytesMax
    if constexpr (Args::kProfile) lds = FES_LOAD_TABLES_LDS ? a.q.lds_doubles * sizeof(double) : 0;
    if constexpr (Args::kRadial) lds = a.q.lds_doubles * sizeof(double);
    load_slots_kernel<T, POS, VEL, Args><<<grid, kLoadThreads, lds, h->stream>>>(a);
}

// the tables of a checked profile in the device buffer (grows to the largest request); q: the kernels' form
// room for `bytes` of tables in the device buffer (grows to the largest request)
static int load_tab_room(fpic_handle* h, size_t bytes)
{
    Diag& g = h->es->diag;
    if (g.load_tab_bytes < bytes) {
        if (g.load_tab) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, hipFree(g.load_tab));
            h->bytes_grid -= g.load_tab_bytes;
            g.load_tab = nullptr;
            g.load_tab_bytes = 0;
        }
        if (int rc = dev_alloc(h, reinterpret_cast<void**>(&g.load_tab), bytes, &h->bytes_grid)) return rc;
        g.load_tab_bytes = bytes;
    }
    return FPIC_OK;
}

static int load_tables(fpic_handle* h, const struct fpic_load_profile& p, fesload::Profile* q)
{
    Diag& g = h->es->diag;
    const size_t bytes = fesload::layout(p, nullptr, nullptr, nullptr) * sizeof(double);
    if (int rc = load_tab_room(h, bytes)) return rc;
    std::vector<double> host(bytes / sizeof(double));
    fesload::layout(p, host.data(), g.load_tab, q);
    HIP_TRY(h, hipMemcpyAsync(g.load_tab, host.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (host is pageable and leaves scope; every load ends synchronised)
    return FPIC_OK;
}

// the same for a checked radial request
static int load_tables(fpic_handle* h, const struct fpic_load_radial& p, const double (&L)[3], fesload::Radial* q)
{
    Diag& g = h->es->diag;
    const size_t bytes = fesload::radial_layout(p, L, nullptr, nullptr, nullptr) * sizeof(double);
    if (int rc = load_tab_room(h, bytes)) return rc;
    std::vector<double> host(bytes / sizeof(double));
    fesload::radial_layout(p, L, host.data(), g.load_tab, q);
    HIP_TRY(h, hipMemcpyAsync(g.load_tab, host.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

template <typename T, typename Args = LoadArgs<T>, typename Tables = fesload::Profile>
static int load_slots(fpic_handle* h, Species& s, const fesload::Rule& r, const Tables* q, uint64_t* loaded)
{
    *loaded = r.count;
    if (!r.count) return FPIC_OK;
    Args a{};
    if constexpr (Args::kProfile || Args::kRadial) a.q = *q;
    a.slab = static_cast<T*>(s.slab[s.cur]);
    a.id = s.ids_identity ? nullptr : s.id[s.cur];
    a.n_pad = s.n_pad;
    a.s0 = s.ids_identity ? static_cast<size_t>(r.first) : 0;
    a.s1 = s.ids_identity ? static_cast<size_t>(r.first + r.count) : s.n;
    a.r = r;
    const bool pos = r.flags & FPIC_LOAD_POS, vel = r.flags & FPIC_LOAD_VEL;
    if (pos && vel) load_slots_launch<T, true, true, Args>(h, a);
    else if (pos) load_slots_launch<T, true, false, Args>(h, a);
    else load_slots_launch<T, false, true, Args>(h, a);
    HIP_TRY(h, hipGetLastError());
    if (pos) {   // (what set_particles sets after an upload of positions)
        s.binned = false;
        s.census_fresh = s.rebin_pending = s.chunk_census_fresh = false;
        if (h->es->solver != FPIC_SOLVER_NONE) h->es->fields_ready = false;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return FPIC_OK;
}

template <typename T, typename Args = KeepArgs<T>, typename Tables = fesload::Profile>
static int load_keep(fpic_handle* h, Species& s, const fesload::Rule& r, const Tables* q, uint64_t* loaded)
{
    State* st = h->es;
    const Domain& d = *st->dom;
    const bool append = r.flags & FPIC_LOAD_APPEND;
    if (append && s.rebin_pending)
        return fail(h, FPIC_ERR_STATE, ".flags <- FPIC_LOAD_APPEND while a migration rides on the next push: append before the first step or after fpic_sort");
    const size_t base = append ? s.n : 0;
    *loaded = 0;
    size_t kept = 0;
    if (r.count) {
        const size_t nchunks = static_cast<size_t>((r.count + kLoadChunk - 1) / kLoadChunk);
        // the chunks' counts, then 8 bytes for the total (the selection's buffer: grows to the largest request)
        const size_t total_at = (nchunks * sizeof(uint32_t) + 15) / 16 * 16;
        if (int rc = select_buffer(h, total_at + 16)) return rc;
        unsigned char* dev = static_cast<unsigned char*>(st->diag.sel);
        Args a{};
        if constexpr (Args::kProfile || Args::kRadial) a.q = *q;
        a.slab = static_cast<T*>(s.slab[s.cur]);
        a.id = s.id[s.cur];
        a.n_pad = s.n_pad;
        a.base = base;
        a.limit = s.cap;
        a.chunk = reinterpret_cast<uint32_t*>(dev);
        a.nchunks = nchunks;
        a.nz = st->nz; a.z0 = d.z0; a.nzl = d.nzl;
        a.r = r;
        unsigned long long* total = reinterpret_cast<unsigned long long*>(dev + total_at);
        const unsigned grid = static_cast<unsigned>(std::min<size_t>(kLoadBlocks, nchunks));
        size_t lds = 0;   // (as load_slots_launch)
        if constexpr (Args::kProfile) lds = FES_LOAD_TABLES_LDS ? a.q.lds_doubles * sizeof(double) : 0;
        if constexpr (Args::kRadial) lds = a.q.lds_doubles * sizeof(double);
        load_keep_kernel<T, false, Args><<<grid, kLoadThreads, lds, h->stream>>>(a);
        load_scan_kernel<<<1, 1024, 0, h->stream>>>(a.chunk, nchunks, total);
        HIP_TRY(h, hipGetLastError());
        unsigned long long got = 0;
        HIP_TRY(h, hipMemcpyAsync(&got, total, sizeof(got), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (got > s.cap - std::min(base, s.cap) || base > s.cap)
            return fail(h, FPIC_ERR_INVALID_ARG, ".count <- rank %d would hold %llu particles of species %d, its capacity is %zu; nothing was changed", d.rank,
                        static_cast<unsigned long long>(base + got), static_cast<int>(&s - st->sp.data()), s.cap);
        kept = static_cast<size_t>(got);
        if (kept) load_keep_kernel<T, true, Args><<<grid, kLoadThreads, lds, h->stream>>>(a);
        HIP_TRY(h, hipGetLastError());
    }
    // the state domain_set_particles leaves: the live set holds the particles in slot order with their ids, the other set's
    // ids are the slot numbers (the next binning writes both anew)
    s.n = base + kept;
    if (s.n) iota3_kernel<<<blocks_for(s.n), 256, 0, h->stream>>>(s.id[s.cur ^ 1], s.n, 0u);
    HIP_TRY(h, hipGetLastError());
    s.ids_identity = !append && r.first == 0 && kept == r.count;   // (everything kept from id 0 on: slot = id)
    s.binned = false;
    s.census_fresh = s.rebin_pending = s.chunk_census_fresh = false;
    if (st->solver != FPIC_SOLVER_NONE) st->fields_ready = false;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *loaded = kept;
    return FPIC_OK;
}

int load(fpic_handle* h, const fpic_load_spec* spec, uint64_t* loaded) { return load_profile(h, spec, nullptr, loaded); }

int load_profile(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_profile* profile, uint64_t* loaded)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    State* st = h->es;
    const bool decomposed = st->dom != nullptr;
    const double L[3] = { st->lx, st->ly, st->lz };
    const int nsp = static_cast<int>(st->sp.size());
    const uint64_t have = decomposed || spec->species < 0 || spec->species >= nsp ? ~0ull : st->sp[spec->species].n;
    if (const char* why = fesload::check(*spec, nsp, have, L, decomposed)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (profile)
        if (const char* why = fesload::check_profile(*profile)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    Species& s = st->sp[spec->species];
    if (int rc0 = refuse_thinned(h, s, "fpic_load")) return rc0;
    const fesload::Rule r = fesload::rule_of(*spec, have, L);
    uint64_t done = 0;
    int rc;
    const fesload::Profile* const none = nullptr;
    if (profile && fesload::any_table(*profile)) {
        fesload::Profile q;
        if (int rc0 = load_tables(h, *profile, &q)) return rc0;
        if (decomposed) rc = h->prec == FPIC_F32 ? load_keep<float, KeepProfileArgs<float>>(h, s, r, &q, &done) : load_keep<double, KeepProfileArgs<double>>(h, s, r, &q, &done);
        else rc = h->prec == FPIC_F32 ? load_slots<float, LoadProfileArgs<float>>(h, s, r, &q, &done) : load_slots<double, LoadProfileArgs<double>>(h, s, r, &q, &done);
    } else if (decomposed) rc = h->prec == FPIC_F32 ? load_keep<float>(h, s, r, none, &done) : load_keep<double>(h, s, r, none, &done);
    else rc = h->prec == FPIC_F32 ? load_slots<float>(h, s, r, none, &done) : load_slots<double>(h, s, r, none, &done);
    if (rc == FPIC_OK && loaded) *loaded = done;
    return rc;
}

int load_radial(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_radial* radial, uint64_t* loaded)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (!radial) return fail(h, FPIC_ERR_INVALID_ARG, ".radial <- Non-optional property is undefined!");
    State* st = h->es;
    const bool decomposed = st->dom != nullptr;
    const double L[3] = { st->lx, st->ly, st->lz };
    const int nsp = static_cast<int>(st->sp.size());
    const uint64_t have = decomposed || spec->species < 0 || spec->species >= nsp ? ~0ull : st->sp[spec->species].n;
    if (const char* why = fesload::check(*spec, nsp, have, L, decomposed)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fesload::check_radial(*radial, L)) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    Species& s = st->sp[spec->species];
    if (int rc0 = refuse_thinned(h, s, "fpic_load_radial")) return rc0;
    const fesload::Rule r = fesload::rule_of(*spec, have, L);
    fesload::Radial q;
    if (int rc0 = load_tables(h, *radial, L, &q)) return rc0;
    uint64_t done = 0;
    int rc;
    if (decomposed) rc = h->prec == FPIC_F32 ? load_keep<float, KeepRadialArgs<float>>(h, s, r, &q, &done) : load_keep<double, KeepRadialArgs<double>>(h, s, r, &q, &done);
    else rc = h->prec == FPIC_F32 ? load_slots<float, LoadRadialArgs<float>>(h, s, r, &q, &done) : load_slots<double, LoadRadialArgs<double>>(h, s, r, &q, &done);
    if (rc == FPIC_OK && loaded) *loaded = done;
    return rc;
}
