// fes_series.inc.hpp: the series diagnostic of a CART3D handle (fpic_series_now, fpic_series_record, fpic_series_history) —
// part of fes_api.hip's translation unit (included there after fes_mom.inc.hpp, inside namespace fes).  The rules are
// fes_series_core.hpp, the two passes fes_series_kernels.hpp.
//
// A request is checked, its tracers sorted per species and their filters built on the host once (series_upload), and kept on
// the device in one allocation.  A row is enqueued on the handle's stream: the row is zeroed, the point pass writes the
// entries of the points whose cell plane this handle owns, one tracer pass per species that has tracers writes the entries
// of the tracers whose live slot it holds — to a scratch row (fpic_series_now) or to the recording ring (the hook
// diag_after_substep; no host synchronisation, no collective; the recorder is fes_record.inc.hpp).  GLOBAL on a rank with a
// communicator gathers the ranks' rows in chunks of kSeriesGatherEntries with diag_gather and every rank takes each entry
// from the rank whose flag is set (fesser::select).

constexpr size_t kSeriesGatherEntries = size_t(1) << 14;   // 1 MiB per rank and chunk

static int series_free(fpic_handle* h, SeriesReq& q)
{
    if (q.block) {
        HIP_TRY(h, hipFree(q.block));
        h->bytes_grid -= q.bytes;
    }
    q = SeriesReq();
    return FPIC_OK;
}

// checks `spec` against the handle and builds its device copies into `q` (empty before)
template <typename T>
static int series_upload(fpic_handle* h, const fpic_series_spec& spec, SeriesReq& q)
{
    State* st = h->es;
    std::vector<uint64_t> counts;
    for (const Species& sp : st->sp) counts.push_back(id_span_of(sp));   // (a thinned species keeps ids up to its span)
    if (const char* why = fesser::check(spec, static_cast<int>(st->sp.size()), st->dom ? nullptr : counts.data())) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    if (spec.npoints) {
        if (!st->fields_ready) return fail(h, FPIC_ERR_STATE, "series of points before precalc(): the fields of the current particle positions have not been computed");
        const Domain* d = st->dom;
        const fesdiag::Owned own = fesdiag::owned_planes(st->nz, d ? d->world : 1, d ? d->rank : 0);
        if (!fesdiag::owned_are_held(own, held_of(st), st->nz, true))
            return fail(h, FPIC_ERR_STATE, "a point in the top cell plane of the slab [%d, %d) reads the plane above it, which this handle does not hold: decompose with ghost_planes >= 1",
                        own.k0, own.k0 + own.nk);
    }
    // the block: the points' coordinates (padded to 16 bytes), then per table sorted, index, filter (uint32 each)
    const std::vector<fesser::Table> tables = fesser::build(spec);
    const size_t pts_bytes = (static_cast<size_t>(spec.npoints) * 3 * sizeof(T) + 15) / 16 * 16;
    size_t words = 0;
    for (const fesser::Table& t : tables) words += 2 * t.sorted.size() + t.filter.size();
    std::vector<unsigned char> host(pts_bytes + words * sizeof(uint32_t), 0);
    T* u = reinterpret_cast<T*>(host.data());
    const double len[3] = { st->lx, st->ly, st->lz };
    for (uint32_t p = 0; p < spec.npoints; ++p)
        for (int a = 0; a < 3; ++a) u[3 * p + a] = static_cast<T>(fesser::unit_of(spec.points[3 * p + a], len[a]));
    void* block = nullptr;
    if (int rc = dev_alloc(h, &block, host.size(), &h->bytes_grid)) return rc;
    q.block = block;
    q.bytes = host.size();
    q.npoints = spec.npoints;
    q.ntracers = spec.ntracers;
    uint32_t* at = reinterpret_cast<uint32_t*>(host.data() + pts_bytes);
    const uint32_t* dev = reinterpret_cast<const uint32_t*>(static_cast<unsigned char*>(block) + pts_bytes);
    for (const fesser::Table& t : tables) {
        const size_t m = t.sorted.size();
        std::memcpy(at, t.sorted.data(), m * sizeof(uint32_t));
        std::memcpy(at + m, t.index.data(), m * sizeof(uint32_t));
        std::memcpy(at + 2 * m, t.filter.data(), t.filter.size() * sizeof(uint32_t));
        q.tables.push_back(SeriesTable{ t.species, static_cast<uint32_t>(m), t.log2bits, dev, dev + m, dev + 2 * m });
        at += 2 * m + t.filter.size();
        dev += 2 * m + t.filter.size();
    }
    // (synchronous: the staging vector goes out of scope)
    hipError_t e = hipMemcpyAsync(block, host.data(), host.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)series_free(h, q);
        return fail(h, FPIC_ERR_HIP, "the upload of a series request failed: %s", hipGetErrorString(e));
    }
    return FPIC_OK;
}

// the row of the handle's state now, written to `row` (device memory, q.width() doubles) on the handle's stream
template <typename T>
static int series_enqueue(fpic_handle* h, const SeriesReq& q, double* row)
{
    State* st = h->es;
    HIP_TRY(h, hipMemsetAsync(row, 0, q.width() * sizeof(double), h->stream));
    const Domain* d = st->dom;
    if (q.npoints) {
        const fesdiag::Owned own = fesdiag::owned_planes(st->nz, d ? d->world : 1, d ? d->rank : 0);
        series_points_kernel<T><<<blocks_for(q.npoints), 256, 0, h->stream>>>(static_cast<const T*>(q.block), q.npoints, static_cast<const T*>(st->E4),
                                                                            static_cast<const T*>(st->B4n), st->nx, st->ny, st->nz, held_of(st), own.k0, own.nk, row);
    }
    for (const SeriesTable& t : q.tables) {
        const Species& sp = st->sp[t.species];
        if (!sp.n) continue; // (nothing is read)
        SeriesTracerArgs<T> a{};
        a.id = sp.id[sp.cur];
        a.slab = static_cast<const T*>(sp.slab[sp.cur]);
        a.n = sp.n;
        a.n_pad = sp.n_pad;
        a.sorted = t.sorted;
        a.index = t.index;
        a.filter = t.filter;
        a.m = t.m;
        a.log2bits = t.log2bits;
        a.dead = d ? 1 : 0;
        a.rows = row + static_cast<size_t>(q.npoints) * fesser::kEntry;
        const size_t nv = (sp.n + 3) / 4;
        const unsigned blocks = static_cast<unsigned>(std::min<size_t>(kSeriesBlocks, (nv + kSeriesThreads - 1) / kSeriesThreads));
        series_tracers_kernel<T><<<blocks, kSeriesThreads, (size_t(1) << t.log2bits) / 8, h->stream>>>(a);
    }
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

template <typename T>
static int series_prepare(fpic_handle* h)
{
    return set_lds(series_tracers_kernel<T>, (size_t(1) << fesser::kFilterMaxLog2) / 8) == hipSuccess
               ? FPIC_OK
               : fail(h, FPIC_ERR_HIP, "hipFuncSetAttribute failed for the tracer pass");
}

// entries [0, entries) of `rows` rows of this rank (mine: [rows][entries][8]) against the other ranks': out gets the selection
static int series_select_ranks(fpic_handle* h, const double* mine, size_t total_entries, int flag, double* out)
{
    std::vector<unsigned char> all;
    for (size_t at = 0; at < total_entries; at += kSeriesGatherEntries) {
        const size_t m = std::min(kSeriesGatherEntries, total_entries - at);
        if (int rc = diag_gather(h, mine + at * fesser::kEntry, m * fesser::kEntry * sizeof(double), all)) return rc;
        const int64_t twice = fesser::select(reinterpret_cast<const double*>(all.data()), m * fesser::kEntry, h->comm->world, m, flag, out + at * fesser::kEntry);
        if (twice >= 0)
            return fail(h, FPIC_ERR_STATE, "internal error: two ranks report entry %llu of a series row (%s)", static_cast<unsigned long long>(at + twice),
                        flag == fesser::kPointFlag ? "a point" : "a tracer");
    }
    return FPIC_OK;
}

// rows [rows][npoints + ntracers][8] as they lie in a ring row -> the caller's two arrays, selected over the ranks if collective
static int series_deliver(fpic_handle* h, const SeriesReq& q, const double* mine, size_t rows, bool collective, double* points_out, double* tracers_out)
{
    const size_t P = q.npoints, M = q.ntracers, E = fesser::kEntry;
    std::vector<double> pts(rows * P * E), trs(rows * M * E);
    for (size_t r = 0; r < rows; ++r) {
        if (P) std::memcpy(pts.data() + r * P * E, mine + r * (P + M) * E, P * E * sizeof(double));
        if (M) std::memcpy(trs.data() + r * M * E, mine + (r * (P + M) + P) * E, M * E * sizeof(double));
    }
    if (!collective) {
        if (P && rows) std::memcpy(points_out, pts.data(), pts.size() * sizeof(double));
        if (M && rows) std::memcpy(tracers_out, trs.data(), trs.size() * sizeof(double));
        return FPIC_OK;
    }
    if (P && rows)
        if (int rc = series_select_ranks(h, pts.data(), rows * P, fesser::kPointFlag, points_out)) return rc;
    if (M && rows)
        if (int rc = series_select_ranks(h, trs.data(), rows * M, fesser::kTracerFlag, tracers_out)) return rc;
    return FPIC_OK;
}

int series_now(fpic_handle* h, const fpic_series_spec* spec, int scope, double* points_out, double* tracers_out)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (spec->npoints && !points_out) return fail(h, FPIC_ERR_INVALID_ARG, ".points_out <- Non-optional property is undefined!");
    if (spec->ntracers && !tracers_out) return fail(h, FPIC_ERR_INVALID_ARG, ".tracers_out <- Non-optional property is undefined!");
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    const bool f32 = h->prec == FPIC_F32;
    if (int rc = f32 ? series_prepare<float>(h) : series_prepare<double>(h)) return rc;
    SeriesReq q;
    int rc = f32 ? series_upload<float>(h, *spec, q) : series_upload<double>(h, *spec, q);
    std::vector<double> mine;
    if (rc == FPIC_OK)
        rc = rec_row_now(h, q.width() * sizeof(double), "series",
                         [&](void* row) { return f32 ? series_enqueue<float>(h, q, static_cast<double*>(row)) : series_enqueue<double>(h, q, static_cast<double*>(row)); }, mine);
    if (rc == FPIC_OK) rc = series_deliver(h, q, mine.data(), 1, collective, points_out, tracers_out);
    const int rc2 = series_free(h, q);
    return rc ? rc : rc2;
}

int series_record(fpic_handle* h, const fpic_series_spec* spec, int every, uint32_t capacity)
{
    if (int rc = rec_check(h, every, capacity)) return rc;
    if (every > 0 && !spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    const bool f32 = h->prec == FPIC_F32;
    SeriesReq q;
    if (every > 0) { // (a refused request leaves the recorder as it was)
        if (int rc = f32 ? series_prepare<float>(h) : series_prepare<double>(h)) return rc;
        if (int rc = f32 ? series_upload<float>(h, *spec, q) : series_upload<double>(h, *spec, q)) return rc;
    }
    Diag& g = h->es->diag;
    Recorder& r = g.rec[kRecSeries];
    if (int rc = rec_disarm(h, r, g.series_req.block != nullptr)) return rc;
    if (int rc = series_free(h, g.series_req)) return rc;
    if (!every) return FPIC_OK;
    g.series_req = q;
    const int rc = rec_arm(h, r, every, capacity, q.width() * sizeof(double));
    if (rc) (void)series_free(h, g.series_req);
    return rc;
}

int series_history(fpic_handle* h, int scope, uint64_t* substeps, double* points_out, double* tracers_out, uint64_t capacity, uint64_t* n, uint64_t* dropped)
{
    Diag& g = h->es->diag;
    Recorder& r = g.rec[kRecSeries];
    const char* missing = g.series_req.npoints && !points_out ? "points_out" : g.series_req.ntracers && !tracers_out ? "tracers_out" : nullptr;
    Drain d;
    if (int rc = rec_drain(h, r, scope, !substeps, capacity, missing, n, dropped, d)) return rc;
    if (d.query) return FPIC_OK;
    if (d.cnt)
        if (int rc = series_deliver(h, g.series_req, d.rows.data(), d.cnt, d.collective, points_out, tracers_out)) return rc;
    rec_drained(r, d, substeps, n, dropped);
    return FPIC_OK;
}
