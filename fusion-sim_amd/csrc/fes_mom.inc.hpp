// fes_mom.inc.hpp: the fluid moment grids of a CART3D handle (fpic_moments) — part of fes_api.hip's translation unit
// (included there after fes_hist.inc.hpp, inside namespace fes).  The rule and the checks of a request are
// fes_mom_core.hpp, the passes fes_mom_kernels.hpp.
//
// A call zeroes its buffer (one grid of the planes the handle holds per moment asked for, then the words `rejected` and
// `spilled`) on the handle's stream, launches the sweeps over the species' slots, copies the buffer back and waits.  A binned
// species takes the tiled pass over its live work list, as many moments per sweep as MomWin::kSweep windows of the species'
// tile shape allow (three of 17 x 17 x 9, ten of 9^3), the moments spread evenly over the sweeps; a species that is not binned
// takes the flat pass, and so do the arrivals of a migration that wait in the tail of a binned species' array for the next
// re-binning push.  `out` is whole-grid-shaped: a rank that holds its slab's planes only gets them in their places and zero
// elsewhere.  GLOBAL on a rank with a communicator gathers the ranks' grids and counters in chunks of kHistGatherWords
// and every rank adds them as integers (diag_sum_ranks, fes_record.inc.hpp).

static int mom_buffer(fpic_handle* h, size_t words)
{
    Diag& g = h->es->diag;
    if (g.mom_words >= words) return FPIC_OK;
    if (g.mom) { // (grows to the largest request)
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(g.mom));
        h->bytes_grid -= g.mom_words * sizeof(unsigned long long);
        g.mom = nullptr;
        g.mom_words = 0;
    }
    if (int rc = dev_alloc(h, reinterpret_cast<void**>(&g.mom), words * sizeof(unsigned long long), &h->bytes_grid)) return rc;
    g.mom_words = words;
    return FPIC_OK;
}

template <typename T, int LX, int LY, int LZ>
static int mom_launch_tiles(fpic_handle* h, const MomArgs<T>& a, unsigned items)
{
    using W = MomWin<LX, LY, LZ>;
    const size_t shm = (static_cast<size_t>(a.nm) * W::N + 2) * sizeof(unsigned long long);
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&mom_tiles_kernel<T, LX, LY, LZ>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kMomLdsBudget)));
    mom_tiles_kernel<T, LX, LY, LZ><<<items, kMomThreads, shm, h->stream>>>(a);
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

// the sweeps of one request over the species' slots, into dev: popcount(mask) grids of the held planes, rejected, spilled
template <typename T>
static int mom_enqueue(fpic_handle* h, const fpic_moments_spec& spec, unsigned long long* dev, size_t words)
{
    State* st = h->es;
    const Species& sp = st->sp[spec.species];
    const bool yee = st->solver == FPIC_SOLVER_YEE;
    HIP_TRY(h, hipMemsetAsync(dev, 0, words * sizeof(unsigned long long), h->stream));
    if (!sp.n && !sp.tail_count) return FPIC_OK; // (nothing is read)
    int bits[fesmom::kMoments], total = 0;
    for (int b = 0; b < fesmom::kMoments; ++b)
        if (spec.mask & (1u << b)) bits[total++] = b;
    MomArgs<T> a{};
    a.slab = static_cast<const T*>(sp.slab[sp.cur]);
    a.stride = sp.n_pad;
    a.nx = st->nx; a.ny = st->ny; a.nz = st->nz;
    a.held = held_of(st);
    a.ntx = st->ntx; a.nty = st->nty;
    a.grids = dev;
    a.grid_words = held_nodes(st);
    a.counters = dev + static_cast<size_t>(total) * a.grid_words;
    const bool tiled = sp.binned && sp.n;
    if (tiled) { a.work = sp.work2[sp.wl]; a.nwork = sp.nwork2[sp.wl]; }
    // the flat pass carries any number of moments; the tiled one what its windows allow, spread evenly over the sweeps
    const int fit = !tiled ? total : yee ? MomWin<kEL, EmWin<T>::LY, kEL>::kSweep : MomWin<FES_LTX, FES_LTY, FES_LTZ>::kSweep;
    const int sweeps = (total + fit - 1) / fit;
    for (int s = 0, at = 0; s < sweeps; ++s, at += a.nm) {
        a.nm = total / sweeps + (s < total % sweeps ? 1 : 0);   // (ten moments in four sweeps: 3 + 3 + 2 + 2)
        for (int m = 0; m < a.nm; ++m) { a.bit[m] = bits[at + m]; a.grid[m] = at + m; }
        a.counting = s == 0;
        if (tiled) {
            const unsigned items = static_cast<unsigned>(sp.work_cap);
            if (int rc = yee ? mom_launch_tiles<T, kEL, EmWin<T>::LY, kEL>(h, a, items) : mom_launch_tiles<T, FES_LTX, FES_LTY, FES_LTZ>(h, a, items)) return rc;
        }
        // everything of a species that is not binned; of a binned one the arrivals behind its n slots
        a.first = tiled ? sp.tail_first : 0;
        a.count = tiled ? sp.tail_count : sp.n + sp.tail_count;
        if (a.count) {
            const unsigned blocks = std::min<unsigned>(blocks_for(a.count, kMomFlatThreads), kMomFlatBlocks);
            mom_flat_kernel<T><<<blocks, kMomFlatThreads, 0, h->stream>>>(a);
            HIP_TRY(h, hipGetLastError());
        }
    }
    return FPIC_OK;
}

int moments(fpic_handle* h, const fpic_moments_spec* spec, int scope, int64_t* out, fpic_moments_info* info)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (!out) return fail(h, FPIC_ERR_INVALID_ARG, ".out <- Non-optional property is undefined!");
    if (!info) return fail(h, FPIC_ERR_INVALID_ARG, ".info <- Non-optional property is undefined!");
    State* st = h->es;
    if (const char* why = fesmom::check(*spec, static_cast<int>(st->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    const size_t nm = static_cast<size_t>(fesmom::popcount(spec->mask));
    const size_t plane = static_cast<size_t>(st->nx) * st->ny, held = held_nodes(st), nodes = plane * st->nz;
    const size_t words = nm * held + 2;
    if (int rc = mom_buffer(h, words)) return rc;
    unsigned long long* dev = st->diag.mom;
    if (int rc = h->prec == FPIC_F32 ? mom_enqueue<float>(h, *spec, dev, words) : mom_enqueue<double>(h, *spec, dev, words)) return rc;
    uint64_t counters[2];
    HIP_TRY(h, hipMemcpyAsync(counters, dev + nm * held, sizeof(counters), hipMemcpyDeviceToHost, h->stream));
    if (st->zs0 == 0 && st->nzs == st->nz) {
        HIP_TRY(h, hipMemcpyAsync(out, dev, nm * nodes * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    } else {
        // the held planes zs0, zs0 + 1, ... (periodic) into their places of the whole grid: one run, or two where they wrap
        std::memset(out, 0, nm * nodes * sizeof(int64_t));
        const size_t head = std::min<size_t>(st->nzs, static_cast<size_t>(st->nz - st->zs0));
        for (size_t m = 0; m < nm; ++m) {
            HIP_TRY(h, hipMemcpyAsync(out + m * nodes + st->zs0 * plane, dev + m * held, head * plane * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            if (static_cast<size_t>(st->nzs) > head)
                HIP_TRY(h, hipMemcpyAsync(out + m * nodes, dev + m * held + head * plane, (st->nzs - head) * plane * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *info = fpic_moments_info{};
    if (!collective) {
        info->rejected = counters[0];
        info->spilled = counters[1];
        return FPIC_OK;
    }
    // the ranks' grids, chunk by chunk, then their counters: every rank adds them as integers and gets the same sums
    if (int rc = diag_sum_ranks(h, reinterpret_cast<uint64_t*>(out), nm * nodes)) return rc;
    if (int rc = diag_sum_ranks(h, counters, 2)) return rc;
    info->rejected = counters[0];
    info->spilled = counters[1];
    return FPIC_OK;
}
