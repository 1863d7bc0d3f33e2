// encode_api.inc — encodeFilterSection on the device (included by bloomgpu.hip after crc_consts()).

namespace {

// d_words: device word arena the descriptors' word_off point into.  Caller holds d.mu and has set the device.
int32_t encode_sections_device(Device &d, const uint64_t *d_words, const bsg_filter_desc *desc, uint32_t n_blocks,
                               uint8_t *out_region, uint64_t region_cap, uint64_t *out_sec_off, float *ms)
{
    std::vector<bsg::EncodeInfo> info(n_blocks);
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        bsg::EncodeInfo &e = info[b];
        e = bsg::EncodeInfo{};
        e.begin = total;
        const uint64_t len = section_len(desc + (size_t)b * 3);
        if (len > 0xFFFFFFFFull) return fail(BSG_E_UNSUPPORTED, "section %u exceeds 4 GiB", b);
        e.len = (uint32_t)len;
        e.init_image = len >= 4 ? bsg::crc_init_image(len - 4, crc_consts().x2n) : 0u;
        for (uint32_t c = 0; c < 3; ++c) {
            const bsg_filter_desc &f = desc[(size_t)b * 3 + c];
            if (!f.m) continue;
            e.present |= 1u << c;
            e.src[c] = f.word_off;
            e.m[c] = f.m;
            e.k[c] = f.k;
            e.nw[c] = (uint32_t)((f.m + 63) / 64);
        }
        out_sec_off[b] = total;
        total += len;
    }
    out_sec_off[n_blocks] = total;
    if (total > region_cap) return fail(BSG_E_INVALID, "section region needs %llu bytes, caller gave %llu",
                                        (unsigned long long)total, (unsigned long long)region_cap);
    if (n_blocks == 0) return BSG_OK;
    if (!d.d_crc) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d.d_crc), sizeof(bsg::CrcConsts)));
        HIP_TRY(hipMemcpyAsync(d.d_crc, &crc_consts(), sizeof(bsg::CrcConsts), hipMemcpyHostToDevice, d.stream));
    }
    HIP_TRY(d.stage_region.reserve(total + 64));
    Scratch scratch(d);
    bsg::EncodeInfo *d_info = nullptr;
    HIP_TRY(scratch.alloc(&d_info, info.size() * sizeof(bsg::EncodeInfo)));
    HIP_TRY(hipMemcpyAsync(d_info, info.data(), info.size() * sizeof(bsg::EncodeInfo), hipMemcpyHostToDevice, d.stream));
    EventList ev;                          // start / stop of the two dispatches
    HIP_TRY(ev.add(4));
    hipExtLaunchKernelGGL(bsg::k_encode_payload, dim3(n_blocks), dim3(256), 0, d.stream, ev.v[0], ev.v[1], 0, d_words,
                          (const bsg::EncodeInfo *)d_info, d.stage_region.p);
    hipExtLaunchKernelGGL(bsg::k_crc_sections, dim3(n_blocks), dim3(bsg::kDecodeThreads), 0, d.stream, ev.v[2], ev.v[3], 0,
                          d.stage_region.p, (const bsg::EncodeInfo *)d_info, (const bsg::CrcConsts *)d.d_crc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_region, d.stage_region.p, total, hipMemcpyDeviceToHost, d.stream));
    HIP_TRY(hipStreamSynchronize(d.stream));
    scratch.done();
    float t_payload = 0.f, t_crc = 0.f;
    (void)hipEventElapsedTime(&t_payload, ev.v[0], ev.v[1]);
    (void)hipEventElapsedTime(&t_crc, ev.v[2], ev.v[3]);
    if (ms) *ms = t_payload + t_crc;
    return BSG_OK;
}

}  // namespace

extern "C" {

int32_t bsg_sections_size(const bsg_filter_desc *desc, uint32_t n_blocks, uint64_t *out_total)
{
    if (!out_total || (n_blocks && !desc)) return fail(BSG_E_INVALID, "null argument");
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) total += section_len(desc + (size_t)b * 3);
    *out_total = total;
    return BSG_OK;
}

int32_t bsg_build_sections(bsg_ctx *ctx, const uint8_t *bytes, const uint32_t *offsets, uint32_t n_entries,
                           const uint32_t *filter_entry_start, const bsg_filter_desc *desc, uint32_t n_filters,
                           uint64_t n_words, uint8_t *out_region, uint64_t region_cap, uint64_t *out_sec_off)
{
    if (n_filters % 3 != 0) return fail(BSG_E_INVALID, "n_filters must be a multiple of 3 (field, token, field::token per block)");
    if (!out_region || !out_sec_off) return fail(BSG_E_INVALID, "null argument");
    SectionsOut so{out_region, region_cap, out_sec_off};
    return build_common(ctx, bytes, offsets, nullptr, n_entries, filter_entry_start, desc, n_filters, nullptr, n_words, &so);
}

int32_t bsg_last_encode_ms(bsg_ctx *ctx, float *encode_ms)
{
    BSG_ENTER(ctx);
    if (!ctx || !encode_ms) return fail(BSG_E_INVALID, "null argument");
    std::lock_guard<std::shared_mutex> lk(ctx->mu);
    *encode_ms = ctx->last_encode_ms;
    return BSG_OK;
}

}  // extern "C"
