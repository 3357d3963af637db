// C-ABI of libtmhip.so (include/tmhip.h): the illuminati chain: align / scale / clip and the
// fused correct -> align -> clip -> scale pass.
#include "abi_internal.h"

namespace tmh {

static void check_windows(const tmh_window* w, int64_t n, int H, int W, int oh, int ow) {
  for (int64_t i = 0; i < n; ++i) {
    const tmh_window& x = w[i];
    TMH_CHECK(x.rows >= 0 && x.cols >= 0, TMH_EINVAL, "alignment window has negative extent");
    if (x.rows == 0 || x.cols == 0) continue;
    TMH_CHECK(x.src_r0 >= 0 && x.src_c0 >= 0 && x.src_r0 + x.rows <= H && x.src_c0 + x.cols <= W,
              TMH_EINVAL, "alignment window leaves the source image");
    TMH_CHECK(x.dst_r0 >= 0 && x.dst_c0 >= 0 && x.dst_r0 + x.rows <= oh && x.dst_c0 + x.cols <= ow,
              TMH_EINVAL, "alignment window leaves the output image");
  }
}

static void check_scale(int lo, int hi) {
  TMH_CHECK(lo >= 0 && lo < 65536 && hi >= 0 && hi < 65536, TMH_EINVAL,
            "scale bounds must be in the range [0, 65535]");
  TMH_CHECK(lo < hi, TMH_EINVAL, "\"lower_bound\" must be smaller than \"upper_bound\"");
}

static void correct_chain_u8_dev(tmh_corrector* c, const uint16_t* dev_in, uint8_t* dev_out,
                                 int64_t n_sites, const tmh_window* host_windows, int clip_lo,
                                 int clip_hi, void* stream) {
  TMH_CHECK(c && n_sites >= 0 && ((dev_in && dev_out && host_windows) || n_sites == 0),
            TMH_EINVAL, "bad arguments");
  check_scale(clip_lo, clip_hi);
  check_windows(host_windows, n_sites, c->H, c->W, c->H, c->W);
  TMH_CHECK(!c->log_transform || (c->zero_log10 >= -37.0 && c->zero_log10 <= 0.0), TMH_EINVAL,
            "the chain pass needs zero_log10 in [-37, 0]");
  if (n_sites == 0) return;
  hipStream_t s = pick(c->stream, stream);
  if ((size_t)n_sites > c->win.n) {
    TMH_HIP(hipStreamSynchronize(s));
    c->win.alloc((size_t)n_sites);
  }
  TMH_HIP(hipMemcpyAsync(c->win.p, host_windows, (size_t)n_sites * sizeof(tmh_window),
                         hipMemcpyHostToDevice, s));
  const FixList fl = corrector_fixlist(c, n_sites, s);
  if (!c->lut8.n) c->lut8.alloc(65536);
  corrector_forms(c, s);
  launch_chain_u8(dev_in, dev_out, c->H, c->W, n_sites, c->coef_lin.p, c->mconst2.p, fl,
                  c->coef64.p, c->rc.p, c->log_transform, c->win.p, clip_lo, clip_hi,
                  c->lut8.p, s, c->zero_log10);
  TMH_HIP(hipStreamSynchronize(s));  // the window buffer is reused by the next call
}

// argument checks of the jterator channel stack, and its device table
// (launch_stack_u16): plane of each (site, slot), site and slot of each plane,
// the planes' windows
static std::vector<int32_t> stack_table(tmh_corrector* c, const void* in, const void* out,
                                        int64_t n_planes, int H, int W, const int32_t* site,
                                        const int32_t* slot, const tmh_window* win,
                                        int64_t n_sites, int slots, int out_h, int out_w) {
  TMH_CHECK(n_planes >= 0 && n_sites >= 0 && slots >= 1 && H > 0 && W > 0 && out_h >= 0 &&
                out_w >= 0,
            TMH_EINVAL, "bad arguments");
  TMH_CHECK(n_planes == 0 || (in && site && slot && win), TMH_EINVAL, "bad arguments");
  TMH_CHECK(out || n_sites == 0 || out_h == 0 || out_w == 0, TMH_EINVAL, "bad arguments");
  TMH_CHECK(n_sites <= 65535, TMH_EINVAL, "at most 65,535 sites per stack call");
  TMH_CHECK(n_sites * slots < ((int64_t)1 << 31), TMH_EINVAL, "too many (site, slot) pairs");
  TMH_CHECK((int64_t)out_h * out_w <= (int64_t)65535 * 2048, TMH_EINVAL,
            "at most 65,535 x 2,048 pixels per aligned site");
  TMH_CHECK(!c || (c->H == H && c->W == W), TMH_EINVAL,
            "the corrector was made for another image size");
  std::vector<int32_t> t((size_t)(n_sites * slots + 8 * n_planes), -1);
  int32_t* site_of = t.data() + n_sites * slots;
  int32_t* slot_of = site_of + n_planes;
  tmh_window* w = reinterpret_cast<tmh_window*>(slot_of + n_planes);
  for (int64_t p = 0; p < n_planes; ++p) {
    TMH_CHECK(site[p] >= 0 && site[p] < n_sites, TMH_EINVAL, "site index out of range");
    TMH_CHECK(slot[p] >= 0 && slot[p] < slots, TMH_EINVAL, "slot index out of range");
    int32_t& owner = t[(size_t)site[p] * slots + slot[p]];
    TMH_CHECK(owner < 0, TMH_EINVAL, "two planes map to one (site, slot)");
    owner = (int32_t)p;
    TMH_CHECK(win[p].rows == out_h && win[p].cols == out_w, TMH_EINVAL,
              "could not broadcast a window's extent into the stack's (out_h, out_w)");
    TMH_CHECK(win[p].src_r0 >= 0 && win[p].src_c0 >= 0 &&
                  (int64_t)win[p].src_r0 + out_h <= H && (int64_t)win[p].src_c0 + out_w <= W,
              TMH_EINVAL, "alignment window leaves the source image");
    site_of[p] = site[p];
    slot_of[p] = slot[p];
    w[p] = win[p];
  }
  return t;
}

static void correct_stack_u16_dev(tmh_corrector* c, const uint16_t* dev_in, uint16_t* dev_out,
                                  int64_t n_planes, int H, int W, const int32_t* host_site,
                                  const int32_t* host_slot, const tmh_window* host_windows,
                                  int64_t n_sites, int slots, int out_h, int out_w, void* stream) {
  const std::vector<int32_t> t = stack_table(c, dev_in, dev_out, n_planes, H, W, host_site,
                                             host_slot, host_windows, n_sites, slots, out_h, out_w);
  if (n_sites == 0 || out_h == 0 || out_w == 0) return;
  // the f64 fixup re-reads the planes after the stack is stored (and the pass
  // gathers from planes other workgroups may have written over): input and
  // output must not overlap
  const uint16_t* in_end = dev_in + n_planes * (int64_t)H * W;
  const uint16_t* out_end = dev_out + n_sites * (int64_t)out_h * out_w * slots;
  TMH_CHECK(n_planes == 0 || in_end <= dev_out || out_end <= dev_in, TMH_EINVAL,
            "input and output of the stack must not overlap");
  hipStream_t s = pick(c ? c->stream : nullptr, stream);
  const int any_unmapped =
      std::count(t.begin(), t.begin() + n_sites * slots, (int32_t)-1) > 0 ? 1 : 0;
  DBuf<int32_t> tab;
  tab.alloc(t.size());
  TMH_HIP(hipMemcpyAsync(tab.p, t.data(), t.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (c) {
    const FixList fl = corrector_fixlist(c, n_planes, s);
    corrector_forms(c, s);
    launch_stack_u16(dev_in, dev_out, n_planes, H, W, n_sites, slots, out_h, out_w, tab.p,
                     c->coef.p, c->lut.p, c->mconst.p, fl, c->coef64.p, c->rc.p, c->log_transform,
                     any_unmapped, s);
  } else {
    launch_stack_u16(dev_in, dev_out, n_planes, H, W, n_sites, slots, out_h, out_w, tab.p, nullptr,
                     nullptr, nullptr, FixList{nullptr, nullptr, 0u}, nullptr, nullptr, 0,
                     any_unmapped, s);
  }
  TMH_HIP(hipStreamSynchronize(s));  // the table is freed on return
}

}  // namespace tmh

extern "C" {

int tmh_correct_stack_u16_device(tmh_corrector* c, const uint16_t* dev_in, uint16_t* dev_out,
                                 int64_t n_planes, int height, int width,
                                 const int32_t* host_site, const int32_t* host_slot,
                                 const tmh_window* host_windows, int64_t n_sites, int slots,
                                 int out_h, int out_w, void* stream) {
  return guard([&] {
    correct_stack_u16_dev(c, dev_in, dev_out, n_planes, height, width, host_site, host_slot,
                          host_windows, n_sites, slots, out_h, out_w, stream);
  });
}

int tmh_correct_stack_u16(tmh_corrector* c, const uint16_t* host_in, uint16_t* host_out,
                          int64_t n_planes, int height, int width, const int32_t* host_site,
                          const int32_t* host_slot, const tmh_window* host_windows,
                          int64_t n_sites, int slots, int out_h, int out_w) {
  return guard([&] {
    // (checked before anything is uploaded; the shared body checks again)
    stack_table(c, host_in, host_out, n_planes, height, width, host_site, host_slot, host_windows,
                n_sites, slots, out_h, out_w);
    const size_t out_n = (size_t)n_sites * out_h * out_w * slots;
    if (out_n == 0) return;
    DBuf<uint16_t> a, b;
    if (n_planes > 0) a.upload(host_in, (size_t)n_planes * height * width);
    b.alloc(out_n);
    correct_stack_u16_dev(c, a.p, b.p, n_planes, height, width, host_site, host_slot, host_windows,
                          n_sites, slots, out_h, out_w, nullptr);
    b.download(host_out, out_n);
  });
}

int tmh_align(const void* host_in, void* host_out, int elem_bytes, int64_t n_sites, int height,
              int width, const tmh_window* windows, int out_height, int out_width) {
  return guard([&] {
    TMH_CHECK((elem_bytes == 1 || elem_bytes == 2) && n_sites >= 0 && height > 0 && width > 0 &&
                  out_height >= 0 && out_width >= 0 && (windows || n_sites == 0) &&
                  ((host_in && host_out) || n_sites == 0),
              TMH_EINVAL, "bad arguments");
    check_windows(windows, n_sites, height, width, out_height, out_width);
    if (n_sites == 0) return;
    const size_t in_b = (size_t)n_sites * height * width * elem_bytes;
    const size_t out_b = (size_t)n_sites * out_height * out_width * elem_bytes;
    DBuf<uint8_t> a, b;
    DBuf<tmh_window> w;
    a.upload(host_in, in_b);
    b.alloc(std::max<size_t>(out_b, 1));
    w.upload(windows, (size_t)n_sites);
    launch_align(a.p, b.p, elem_bytes, n_sites, height, width, out_height, out_width, w.p, nullptr);
    TMH_HIP(hipDeviceSynchronize());
    if (out_b) b.download(host_out, out_b);
  });
}

int tmh_map_u16_to_u8(const uint16_t* host_in, uint8_t* host_out, int64_t n, int lower,
                      int upper) {
  return guard([&] {
    TMH_CHECK(n >= 0 && ((host_in && host_out) || n == 0), TMH_EINVAL, "bad arguments");
    check_scale(lower, upper);
    if (n == 0) return;
    DBuf<uint16_t> a;
    DBuf<uint8_t> b;
    a.upload(host_in, (size_t)n);
    b.alloc((size_t)n);
    launch_map_u8(a.p, b.p, n, lower, upper, nullptr);
    TMH_HIP(hipDeviceSynchronize());
    b.download(host_out, (size_t)n);
  });
}

int tmh_clip_u16(const uint16_t* host_in, uint16_t* host_out, int64_t n, int lo, int hi) {
  return guard([&] {
    TMH_CHECK((host_in && host_out) || n == 0, TMH_EINVAL, "bad arguments");
    TMH_CHECK(lo >= 0 && lo <= 65535 && hi >= 0 && hi <= 65535, TMH_EINVAL, "clip bounds out of range");
    if (n == 0) return;
    DBuf<uint16_t> a, b;
    a.upload(host_in, (size_t)n);
    b.alloc(n);
    launch_clip_u16(a.p, b.p, n, lo, hi, nullptr);
    b.download(host_out, (size_t)n);
  });
}

int tmh_correct_chain_u8_device(tmh_corrector* c, const uint16_t* dev_in, uint8_t* dev_out,
                                int64_t n_sites, const tmh_window* host_windows, int clip_lo,
                                int clip_hi, void* stream) {
  return guard([&] {
    correct_chain_u8_dev(c, dev_in, dev_out, n_sites, host_windows, clip_lo, clip_hi, stream);
  });
}

int tmh_correct_chain_u8(tmh_corrector* c, const uint16_t* host_in, uint8_t* host_out,
                         int64_t n_sites, const tmh_window* host_windows, int clip_lo,
                         int clip_hi) {
  return guard([&] {
    TMH_CHECK(c && n_sites >= 0 && ((host_in && host_out && host_windows) || n_sites == 0),
              TMH_EINVAL, "bad arguments");
    if (n_sites == 0) return;
    const size_t npx = (size_t)c->npx;
    DBuf<uint16_t> a;
    DBuf<uint8_t> b;
    a.alloc((size_t)n_sites * npx);
    b.alloc((size_t)n_sites * npx);
    TMH_HIP(hipMemcpyAsync(a.p, host_in, (size_t)n_sites * npx * 2, hipMemcpyHostToDevice,
                           c->stream));
    correct_chain_u8_dev(c, a.p, b.p, n_sites, host_windows, clip_lo, clip_hi, nullptr);
    b.download(host_out, (size_t)n_sites * npx);
  });
}

}  // extern "C"
