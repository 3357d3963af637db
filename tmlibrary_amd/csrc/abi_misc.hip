// C-ABI of libtmhip.so (include/tmhip.h): synthetic sites, the box probe, site-image input.
#include "abi_internal.h"

extern "C" {

int tmh_synth_sites_device(uint16_t* dev_out, int64_t n_sites, int height, int width, uint64_t seed,
                           int channel, int64_t first_site, int distribution, void* stream) {
  return guard([&] {
    TMH_CHECK(dev_out && n_sites >= 0 && height > 0 && width > 0 && first_site >= 0, TMH_EINVAL,
              "bad arguments");
    TMH_CHECK(distribution >= TMH_SYNTH_STANDARD && distribution <= TMH_SYNTH_UNIFORM, TMH_EINVAL,
              "unknown distribution");
    if (n_sites == 0) return;
    launch_synth(dev_out, n_sites, height, width, seed, channel, first_site, distribution,
                 (hipStream_t)stream);
  });
}

int tmh_box_probe_device(const uint16_t* const* dev_in_blocks, uint16_t* const* dev_out_blocks,
                         int block_shift, int64_t n_sites, int height, int width, int mode,
                         int reps, void* stream, double* ms_out, double* sclk_mhz_out) {
  return guard([&] {
    TMH_CHECK(dev_in_blocks && n_sites > 0 && n_sites < (int64_t(1) << 24) && height > 0 &&
                  width > 0 && ((int64_t)height * width) % 8 == 0 && block_shift >= 0 &&
                  block_shift <= 24 && mode >= 0 && mode <= 3 && reps > 0 && ms_out,
              TMH_EINVAL, "bad arguments");
    const bool write = (mode & 1) == 0, flat = mode >= 2;
    TMH_CHECK(!write || dev_out_blocks, TMH_EINVAL, "the copy probe needs output blocks");
    const hipStream_t s = (hipStream_t)stream;
    int dev = 0, cus = 0;
    TMH_HIP(hipGetDevice(&dev));
    TMH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    DBuf<unsigned long long> clk;
    DBuf<unsigned int> sink;
    clk.alloc(4);
    sink.alloc(1);
    hipEvent_t e0, e1;
    TMH_HIP(hipEventCreate(&e0));
    TMH_HIP(hipEventCreate(&e1));
    const int64_t npx = (int64_t)height * width;
    const int64_t per = (int64_t)1 << block_shift, nb = (n_sites + per - 1) / per;
    std::vector<const uint16_t*> hin;
    std::vector<uint16_t*> hout;
    if (flat) {  // the flat shape launches per block: the block pointers on the host
      hin.resize(nb);
      TMH_HIP(hipMemcpy(hin.data(), dev_in_blocks, nb * sizeof(void*), hipMemcpyDeviceToHost));
      if (write) {
        hout.resize(nb);
        TMH_HIP(hipMemcpy(hout.data(), dev_out_blocks, nb * sizeof(void*), hipMemcpyDeviceToHost));
      }
    }
    TMH_HIP(hipMemsetAsync(clk.p, 0, 4 * sizeof(unsigned long long), s));
    float ms = 0.0f;
    try {
      TMH_HIP(hipEventRecord(e0, s));
      for (int r = 0; r < reps; ++r) {
        if (!flat) {
          launch_box_probe(dev_in_blocks, const_cast<uint16_t* const*>(dev_out_blocks),
                           block_shift, n_sites, npx, write, clk.p, sink.p, cus, s);
          continue;
        }
        for (int64_t b = 0; b < nb; ++b)
          launch_box_probe_flat(hin[b], write ? hout[b] : nullptr,
                                std::min<int64_t>(per, n_sites - b * per), npx, write, sink.p, s);
      }
      TMH_HIP(hipEventRecord(e1, s));
      TMH_HIP(hipEventSynchronize(e1));
      TMH_HIP(hipEventElapsedTime(&ms, e0, e1));
    } catch (...) {
      (void)hipStreamSynchronize(s);  // no launch left using clk / sink as they unwind
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_out = (double)ms / reps;
    if (sclk_mhz_out) {
      unsigned long long t[4];
      TMH_HIP(hipMemcpy(t, clk.p, sizeof(t), hipMemcpyDeviceToHost));
      *sclk_mhz_out = t[3] > t[1] ? 100.0 * (double)(t[2] - t[0]) / (double)(t[3] - t[1]) : 0.0;
    }
  });
}

int tmh_synth_tables(int distribution, int height, int width, int32_t* ln16, int32_t* nz16,
                     int32_t* ey, int32_t* ex) {
  return guard([&] {
    TMH_CHECK(ln16 && nz16 && ey && ex && height > 0 && width > 0, TMH_EINVAL, "bad arguments");
    TMH_CHECK(distribution >= TMH_SYNTH_STANDARD && distribution <= TMH_SYNTH_UNIFORM, TMH_EINVAL,
              "unknown distribution");
    synth_tables_host(distribution, height, width, ln16, nz16, ey, ex);
  });
}

int64_t tmh_inflate_scratch_bytes(int64_t n_chunks, int64_t raw_max) {
  return n_chunks > 0 && raw_max >= 0 ? inflate_scratch_bytes(n_chunks, raw_max) : 0;
}

int tmh_inflate_device(const uint8_t* dev_src, int64_t src_bytes, const tmh_zchunk* dev_chunks,
                       int64_t n_chunks, int64_t raw_max, uint8_t* dev_raw, int64_t raw_bytes,
                       void* dev_scratch, int64_t scratch_bytes, int32_t* dev_status,
                       void* stream) {
  return guard([&] {
    TMH_CHECK(n_chunks >= 0 && src_bytes >= 0 && raw_bytes >= 0 && raw_max >= 0, TMH_EINVAL,
              "bad sizes");
    if (n_chunks == 0) return;
    TMH_CHECK(dev_src && dev_chunks && dev_raw && dev_status && dev_scratch, TMH_EINVAL,
              "bad arguments");
    TMH_CHECK(raw_max < (int64_t(1) << 31), TMH_EINVAL, "chunks must hold fewer than 2^31 bytes");
    TMH_CHECK(scratch_bytes >= inflate_scratch_bytes(n_chunks, raw_max), TMH_EINVAL,
              "scratch smaller than tmh_inflate_scratch_bytes");
    TMH_CHECK((reinterpret_cast<uintptr_t>(dev_scratch) & 15) == 0, TMH_EINVAL,
              "scratch must be 16-byte aligned");
    launch_inflate(dev_src, src_bytes, dev_chunks, n_chunks, raw_max, dev_raw, raw_bytes,
                   static_cast<uint32_t*>(dev_scratch), dev_status, (hipStream_t)stream);
  });
}

int tmh_place_chunks_device(const uint8_t* dev_raw, const tmh_zchunk* dev_chunks, int64_t n_chunks,
                            int height, int width, int elem_bytes, int chunk_rows, int chunk_cols,
                            void* dev_images, void* stream) {
  return guard([&] {
    TMH_CHECK(n_chunks >= 0 && height > 0 && width > 0 && chunk_rows > 0 && chunk_cols > 0 &&
                  (elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8),
              TMH_EINVAL, "bad geometry");
    if (n_chunks == 0) return;
    TMH_CHECK(dev_raw && dev_chunks && dev_images, TMH_EINVAL, "bad arguments");
    launch_place_chunks(dev_raw, dev_chunks, n_chunks, height, width, elem_bytes, chunk_rows,
                        chunk_cols, static_cast<uint8_t*>(dev_images), (hipStream_t)stream);
  });
}

}  // extern "C"
