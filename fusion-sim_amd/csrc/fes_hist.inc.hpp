// fes_hist.inc.hpp: the phase-space histograms of a CART3D handle (fpic_histogram) — part of fes_api.hip's translation unit
// (included there after fes_diag.inc.hpp, inside namespace fes).  The bin rule and the checks of a request are
// fes_hist_core.hpp, the pass fes_hist_kernels.hpp.
//
// A call zeroes the counters (nbins + 1 words: the bins, then `outside`) on the handle's stream, launches one pass over the
// species' slots, copies the counters back and waits.  The pass keeps a private histogram in LDS when the request has at
// most kHistLdsBins bins and adds to the global counters directly otherwise.  GLOBAL on a rank with a communicator gathers
// the ranks' counters in chunks of kHistGatherWords and every rank adds them as integers (diag_sum_ranks,
// fes_record.inc.hpp): every rank gets the same sums.

static int hist_buffer(fpic_handle* h, size_t words)
{
    Diag& g = h->es->diag;
    if (g.hist_words >= words) return FPIC_OK;
    if (g.hist) { // (grows to the largest request)
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipFree(g.hist));
        h->bytes_grid -= g.hist_words * sizeof(unsigned long long);
        g.hist = nullptr;
        g.hist_words = 0;
    }
    if (int rc = dev_alloc(h, reinterpret_cast<void**>(&g.hist), words * sizeof(unsigned long long), &h->bytes_grid)) return rc;
    g.hist_words = words;
    return FPIC_OK;
}

template <typename T, int K0, int K1>
static int hist_launch(fpic_handle* h, const HistArgs<T>& a, bool lds, unsigned long long* counts)
{
    if (lds) {
        const size_t shm = std::max<size_t>(a.nbins * sizeof(uint32_t), 64);
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&hist_kernel<T, K0, K1, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(kHistLdsBins * sizeof(uint32_t))));
        hist_kernel<T, K0, K1, true><<<kHistBlocks, kHistThreads, shm, h->stream>>>(a, counts);
    } else {
        hist_kernel<T, K0, K1, false><<<kHistBlocks, kHistThreads, 64, h->stream>>>(a, counts);
    }
    HIP_TRY(h, hipGetLastError());
    return FPIC_OK;
}

// the pass of one request over the species' slots, into counts[0 .. nbins] (device memory, zeroed here)
template <typename T>
static int hist_enqueue(fpic_handle* h, const fpic_hist_spec& spec, unsigned long long* counts)
{
    State* st = h->es;
    const Species& sp = st->sp[spec.species];
    HistArgs<T> a{};
    a.n = sp.n;
    a.nbins = static_cast<uint32_t>(spec.bins[0]) * (spec.naxes == 2 ? static_cast<uint32_t>(spec.bins[1]) : 1u);
    HIP_TRY(h, hipMemsetAsync(counts, 0, (static_cast<size_t>(a.nbins) + 1) * sizeof(unsigned long long), h->stream));
    if (!sp.n) return FPIC_OK; // (nothing is read)
    const T* slab = static_cast<const T*>(sp.slab[sp.cur]);
    int kind[2] = { HIST_NONE, HIST_NONE };
    a.dead_from = st->dom ? 2 : -1;
    for (int k = 0; k < spec.naxes; ++k) {
        a.ax[k] = feshist::axis_of(spec, k);
        if (spec.axis[k] == FPIC_AXIS_V2) {
            kind[k] = HIST_V2;
            for (int c = 0; c < 3; ++c) a.src[k][c] = slab + (3 + c) * sp.n_pad;
        } else {
            kind[k] = HIST_PLAIN;
            a.src[k][0] = slab + static_cast<size_t>(spec.axis[k]) * sp.n_pad;   // (the slab's arrays: x, y, z, vx, vy, vz)
            if (st->dom && spec.axis[k] == FPIC_AXIS_X) a.dead_from = k;
        }
    }
    if (a.dead_from == 2) a.x = slab;
    const bool lds = a.nbins <= kHistLdsBins && hist_block_share(sp.n, 16 / sizeof(T)) < (1ull << 32);
    if (kind[1] == HIST_NONE) return kind[0] == HIST_V2 ? hist_launch<T, HIST_V2, HIST_NONE>(h, a, lds, counts) : hist_launch<T, HIST_PLAIN, HIST_NONE>(h, a, lds, counts);
    if (kind[0] == HIST_V2) return hist_launch<T, HIST_V2, HIST_PLAIN>(h, a, lds, counts);
    return kind[1] == HIST_V2 ? hist_launch<T, HIST_PLAIN, HIST_V2>(h, a, lds, counts) : hist_launch<T, HIST_PLAIN, HIST_PLAIN>(h, a, lds, counts);
}

int histogram(fpic_handle* h, const fpic_hist_spec* spec, int scope, uint64_t* counts, uint64_t* outside)
{
    if (!spec) return fail(h, FPIC_ERR_INVALID_ARG, ".spec <- Non-optional property is undefined!");
    if (!counts) return fail(h, FPIC_ERR_INVALID_ARG, ".counts <- Non-optional property is undefined!");
    if (!outside) return fail(h, FPIC_ERR_INVALID_ARG, ".outside <- Non-optional property is undefined!");
    if (const char* why = feshist::check(*spec, static_cast<int>(h->es->sp.size()))) return fail(h, FPIC_ERR_INVALID_ARG, "%s", why);
    bool collective = false;
    if (int rc = diag_scope(h, scope, collective)) return rc;
    const size_t nbins = static_cast<size_t>(spec->bins[0]) * (spec->naxes == 2 ? spec->bins[1] : 1), words = nbins + 1;
    if (int rc = hist_buffer(h, words)) return rc;
    unsigned long long* dev = h->es->diag.hist;
    if (int rc = h->prec == FPIC_F32 ? hist_enqueue<float>(h, *spec, dev) : hist_enqueue<double>(h, *spec, dev)) return rc;
    if (!collective) {
        HIP_TRY(h, hipMemcpyAsync(counts, dev, nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(outside, dev + nbins, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return FPIC_OK;
    }
    std::vector<uint64_t> sum(words);
    HIP_TRY(h, hipMemcpyAsync(sum.data(), dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = diag_sum_ranks(h, sum.data(), words)) return rc;
    std::memcpy(counts, sum.data(), nbins * sizeof(uint64_t));
    *outside = sum[nbins];
    return FPIC_OK;
}
