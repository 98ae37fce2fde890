// fake_kernels.cpp -- every launcher and setup function the host layer calls (kernels.h, strided_kernels.h, fft2d_kernels.h,
// real_kernels.h, conv_kernels.h, stft_kernels.h), simulated: a launcher is an injectable call site that reports to the fake runtime
// (fake_hip.h) which bytes its kernel would read and which it would write.  The regions are written out here from the
// contract in each header's comment -- which element of which buffer a workgroup touches, as (count, stride) dimensions over a
// contiguous piece -- and from nothing the real launchers contain: no device header is included.
#include "../../fft_wgpu_amd/conv/conv_kernels.h"
#include "../../fft_wgpu_amd/csrc/kernels.h"
#include "../../fft_wgpu_amd/fft2d/fft2d_kernels.h"
#include "../../fft_wgpu_amd/real/real_kernels.h"
#include "../../fft_wgpu_amd/stft/stft_kernels.h"
#include "../../fft_wgpu_amd/strided/strided_kernels.h"
#include "fake_hip.h"

using sim::Dim;
using sim::Region;

namespace {

constexpr uint64_t E = 8;  // bytes of a sample {f32 re, f32 im}

// `count` samples at p
Region flat(const void *p, uint64_t count, uint64_t elem = E) { return Region{p, count * elem, {}}; }
// the two-level table of W_T (tables.cpp upload_level): lo has min(T, 1024) entries, hi max(T / 1024, 1)
void level(std::vector<Region> &rd, const void *lo, const void *hi, uint64_t T)
{
    rd.push_back(flat(lo, T < 1024 ? T : 1024));
    rd.push_back(flat(hi, T < 1024 ? 1 : T / 1024));
}
// A column pass over `nt` transforms of an L x pitch matrix (row-major, transforms `sb` samples apart), `w` adjacent columns
// per workgroup: workgroup (i, tile) touches rows r = 0 .. L-1 at base + i*sb + r*pitch + tile*w, w samples each.
Region columns(const void *p, uint64_t nt, uint64_t sb, uint64_t L, uint64_t pitch, uint64_t w)
{
    return Region{p, w * E, {{L, pitch * E}, {pitch / w, w * E}, {nt, sb * E}}};
}

}  // namespace

namespace fwa {

// (kLab = true comes from csrc/lab_present.cpp, linked as it is: the laboratory keys are part of the host layer under test)
size_t ring_ctl_bytes(uint64_t batch) { return sizeof(uint32_t) * (32 + 2 * batch); }  // ticket, error word, two counters per transform

hipError_t setup_small32_kernels() { return sim::setup("setup_small32_kernels"); }
hipError_t setup_rows32_kernels() { return sim::setup("setup_rows32_kernels"); }
hipError_t setup_colsw_kernels() { return sim::setup("setup_colsw_kernels"); }
hipError_t setup_cols32_kernels() { return sim::setup("setup_cols32_kernels"); }
hipError_t setup_tile_kernels() { return sim::setup("setup_tile_kernels"); }
hipError_t setup_1m_kernels() { return sim::setup("setup_1m_kernels"); }
hipError_t setup_p1_gen_kernels() { return sim::setup("setup_p1_gen_kernels"); }
hipError_t setup_lab_1m_kernels() { return sim::setup("setup_lab_1m_kernels"); }

// one stage of the literal recurrence: all of src and the n/2 table in, all of dst out
hipError_t launch_r2_stage(int, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint32_t, uint64_t batch, float, hipStream_t st)
{
    return sim::launch("launch_r2_stage", st, {flat(src, batch * n), flat(tw, n / 2)}, {flat(dst, batch * n)});
}
static hipError_t one_launch(const char *name, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint64_t batch, hipStream_t st)
{
    // batch transforms back to back, each read completely and written completely; the half table of W_n
    return sim::launch(name, st, {Region{src, n * E, {{batch, n * E}}}, flat(tw, n / 2)}, {Region{dst, n * E, {{batch, n * E}}}});
}
hipError_t launch_chunk(int, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint64_t batch, float, hipStream_t st)
{
    return one_launch("launch_chunk", src, dst, tw, n, batch, st);
}
hipError_t launch_small32(int, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint64_t batch, float, hipStream_t st)
{
    return one_launch("launch_small32", src, dst, tw, n, batch, st);
}
hipError_t launch_small16(int, const v2f *src, v2f *dst, const v2f *tw, uint32_t n, uint64_t batch, float, bool, hipStream_t st)
{
    return one_launch("launch_small16", src, dst, tw, n, batch, st);
}

// Last pass of n = n1 * L, L = 2^lg_l.  A workgroup takes R adjacent rows k1 (16; 8 from 2048-point rows on).  in_cw = 0: row k1 is L
// contiguous samples at in + k1*L; in_cw = w: the slab is [tile][k1][w], so row k1 is L / w pieces of w samples, n1*w apart.
// Output sample k2 of row k1 goes to out[k1 + n1*k2]: R adjacent samples per k2.
hipError_t launch_rows32(int, uint32_t lg_l, const v2f *in, v2f *out, const v2f *tw, uint32_t n1, uint64_t in_sb, uint64_t out_sb,
                         uint32_t nt, float, uint32_t, uint32_t in_cw, hipStream_t st)
{
    const uint64_t L = 1ull << lg_l, R = lg_l >= 11 ? 8 : 16;
    Region rd = in_cw == 0 ? Region{in, L * E, {{R, L * E}, {n1 / R, R * L * E}, {nt, in_sb * E}}}
                           : Region{in, in_cw * E, {{R, in_cw * E}, {n1 / R, R * in_cw * E}, {L / in_cw, (uint64_t)n1 * in_cw * E}, {nt, in_sb * E}}};
    Region wr{out, R * E, {{L, (uint64_t)n1 * E}, {n1 / R, R * E}, {nt, out_sb * E}}};
    return sim::launch("launch_rows32", st, {rd, flat(tw, L / 2)}, {wr});
}

// Pass A with short columns in wide tiles: L = 2^lg_l rows x w columns per workgroup, w = 32 at L = 512, 64 at L = 256.  The
// input is the L x pitch matrix; the output the same layout, or tile-contiguous [tile][k1][w].  Twiddles of domain n = L*pitch.
hipError_t launch_colsw(int, uint32_t lg_l, bool tile_ring, const v2f *in, v2f *out, const v2f *tw, const v2f *tw_lo, const v2f *tw_hi,
                        uint32_t pitch, uint64_t in_sb, uint64_t out_sb, uint32_t nt, uint32_t, hipStream_t st)
{
    const uint64_t L = 1ull << lg_l, w = lg_l == 9 ? 32 : 64;
    std::vector<Region> rd = {columns(in, nt, in_sb, L, pitch, w), flat(tw, L / 2)};
    level(rd, tw_lo, tw_hi, L * pitch);
    Region wr = tile_ring ? Region{out, w * E, {{L, w * E}, {pitch / w, L * w * E}, {nt, out_sb * E}}} : columns(out, nt, out_sb, L, pitch, w);
    return sim::launch("launch_colsw", st, rd, {wr});
}
// Pass A with 2048-point columns, 16 adjacent columns per workgroup, matrix layout in and out
hipError_t launch_cols32(int, uint32_t lg_l, const v2f *in, v2f *out, const v2f *tw, const v2f *tw_lo, const v2f *tw_hi, uint32_t pitch,
                         uint64_t in_sb, uint64_t out_sb, uint32_t nt, uint32_t, hipStream_t st)
{
    const uint64_t L = 1ull << lg_l;
    std::vector<Region> rd = {columns(in, nt, in_sb, L, pitch, 16), flat(tw, L / 2)};
    level(rd, tw_lo, tw_hi, L * pitch);
    return sim::launch("launch_cols32", st, rd, {columns(out, nt, out_sb, L, pitch, 16)});
}
// 1024-point column pass, 16-column tiles, run-time pitch; first-stage table [32][32]
hipError_t launch_p1_gen(int, const v2f *src, v2f *dst, const v2f *tw_inner, const v2f *tw_lo, const v2f *tw_hi, uint32_t pitch,
                         uint64_t in_sb, uint64_t out_sb, uint32_t nt, uint32_t, hipStream_t st)
{
    std::vector<Region> rd = {columns(src, nt, in_sb, 1024, pitch, 16), flat(tw_inner, 1024)};
    level(rd, tw_lo, tw_hi, 1024ull * pitch);
    return sim::launch("launch_p1_gen", st, rd, {columns(dst, nt, out_sb, 1024, pitch, 16)});
}

// k_tile.  Workgroup (b, d1, tile) starts at base = b*sb + d1*s1 + tile*st.  COLS: element i of FFT c at base + i*pitch + c, in
// and out, c < cw, i < L; four-step twiddles of domain L*pitch.  ROWS_T: FFT c is the contiguous row at base + c*pitch; output
// o of row c at out base + o*out_stride + c.
hipError_t launch_tile(int, int mode, uint32_t lg_l, const TileArgs &a, uint64_t batch, hipStream_t st)
{
    const uint64_t L = 1ull << lg_l, cw = a.cw;
    auto blocks = [&](uint64_t sb, uint64_t s1, uint64_t stt, std::vector<Dim> inner) {
        inner.push_back({a.tile_count, stt * E});
        inner.push_back({a.d1_count, s1 * E});
        inner.push_back({batch, sb * E});
        return inner;
    };
    std::vector<Region> rd = {flat(a.tw, L / 2)}, wr;
    if (mode == TILE_COLS) {
        rd.push_back(Region{a.in, cw * E, blocks(a.in_sb, a.in_s1, a.in_st, {{L, a.pitch * E}})});
        wr.push_back(Region{a.out, cw * E, blocks(a.out_sb, a.out_s1, a.out_st, {{L, a.pitch * E}})});
        level(rd, a.tw_lo, a.tw_hi, L * a.pitch);
    } else {
        rd.push_back(Region{a.in, L * E, blocks(a.in_sb, a.in_s1, a.in_st, {{cw, a.pitch * E}})});
        wr.push_back(Region{a.out, cw * E, blocks(a.out_sb, a.out_s1, a.out_st, {{L, a.out_stride * E}})});
    }
    return sim::launch("launch_tile", st, rd, wr);
}

// The 2^20 pipeline: transform i of the launch uses ring slot i; 1024 rows x 16-column tiles.  Outer table: per tile A[32][16] and
// B[32][16].
hipError_t launch_p1_1m(int, const v2f *src, v2f *ring, const v2f *tw_inner, const v2f *tw_outer, uint32_t nt, uint32_t, hipStream_t st)
{
    const uint64_t N = 1ull << 20;
    return sim::launch("launch_p1_1m", st, {columns(src, nt, N, 1024, 1024, 16), flat(tw_inner, 1024), flat(tw_outer, 64 * 64 * 16)},
                       {columns(ring, nt, N, 1024, 1024, 16)});
}
hipError_t launch_p2_1m(int, const v2f *ring, v2f *dst, const v2f *tw_inner, uint32_t nt, float, uint32_t, hipStream_t st)
{
    const uint64_t N = 1ull << 20;
    return sim::launch("launch_p2_1m", st, {columns(ring, nt, N, 1024, 1024, 16), flat(tw_inner, 1024)}, {columns(dst, nt, N, 1024, 1024, 16)});
}
hipError_t launch_ring_1m(int, const v2f *src, v2f *dst, v2f *ring, const v2f *tw_inner, const v2f *tw_outer, uint32_t *ctl, uint32_t batch,
                          uint32_t, uint32_t ring_slots, uint32_t, float, hipStream_t st)
{
    const uint64_t N = 1ull << 20;
    // the ring and the control words are written before they are read, inside the launch
    return sim::launch("launch_ring_1m", st, {flat(src, batch * N), flat(tw_inner, 1024), flat(tw_outer, 64 * 64 * 16)},
                       {flat(dst, batch * N), flat(ring, ring_slots * N), flat(ctl, ring_ctl_bytes(batch), 1)});
}

hipError_t launch_scale(const v2f *a, v2f *b, uint64_t n_samples, float, hipStream_t st)
{
    return sim::launch("launch_scale", st, {flat(a, n_samples)}, {flat(b, n_samples)});
}
hipError_t launch_fill(v2f *dst, uint64_t, uint64_t, uint64_t n_samples, float, hipStream_t st)
{
    return sim::launch("launch_fill", st, {}, {flat(dst, n_samples)});
}
hipError_t launch_copy(const void *src, void *dst, uint64_t bytes, hipStream_t st)
{
    return sim::launch("launch_copy", st, {flat(src, bytes, 1)}, {flat(dst, bytes, 1)});
}
hipError_t launch_spin(uint32_t, uint32_t, hipStream_t st) { return sim::launch("launch_spin", st, {}, {}); }

}  // namespace fwa

// every launcher and setup this file defines, by the name it enters the fake with
void sim::declare_launchers()
{
    for (const char *n : {"launch_r2_stage", "launch_chunk", "launch_small32", "launch_small16", "launch_rows32", "launch_colsw", "launch_cols32",
                          "launch_p1_gen", "launch_tile", "launch_p1_1m", "launch_p2_1m", "launch_ring_1m", "launch_scale", "launch_fill",
                          "launch_copy", "launch_spin", "launch_strided", "launch_fft2d_rows", "launch_real", "launch_conv", "launch_stft"})
        sim::declare(n, sim::FN_LAUNCH);
    for (const char *n : {"setup_small32_kernels", "setup_rows32_kernels", "setup_colsw_kernels", "setup_cols32_kernels", "setup_tile_kernels",
                          "setup_1m_kernels", "setup_p1_gen_kernels", "setup_lab_1m_kernels", "setup_strided_kernels", "setup_fft2d_kernels",
                          "setup_real_kernels", "setup_conv_kernels", "setup_stft_kernels"})
        sim::declare(n, sim::FN_OTHER);
}

// ---- the side libraries: one launch each over the whole of their buffers ----
namespace fws {
hipError_t setup_strided_kernels(uint32_t) { return sim::setup("setup_strided_kernels"); }
// columns of `batch` matrices of n rows x howmany columns, in place: tile_cols adjacent columns by all n rows per tile
hipError_t launch_strided(int, uint32_t n, v2f *buf, uint64_t howmany, uint64_t batch, float, hipStream_t st)
{
    const Region r{buf, howmany * E, {{n, howmany * E}, {batch, n * howmany * E}}};
    return sim::launch("launch_strided", st, {r}, {r});
}
}  // namespace fws
namespace fw2 {
hipError_t setup_fft2d_kernels(uint32_t, uint32_t) { return sim::setup("setup_fft2d_kernels"); }
hipError_t launch_fft2d_rows(int, uint32_t rows, uint32_t cols, v2f *buf, uint64_t batch, float, float, hipStream_t st)
{
    const Region r{buf, cols * E, {{batch * rows, cols * E}}};  // every row of every image
    return sim::launch("launch_fft2d_rows", st, {r}, {r});
}
}  // namespace fw2
namespace fwr {
hipError_t setup_real_kernels(uint32_t) { return sim::setup("setup_real_kernels"); }
hipError_t launch_real(int dir, uint32_t n, float *real, float *spec, uint64_t batch, float, hipStream_t st)
{
    const Region re{real, 4ull * n, {{batch, 4ull * n}}}, sp{spec, E * (n / 2 + 1), {{batch, E * (n / 2 + 1)}}};
    return dir == fwa::FWD ? sim::launch("launch_real", st, {re}, {sp}) : sim::launch("launch_real", st, {sp}, {re});
}
}  // namespace fwr
namespace fwc {
hipError_t setup_conv_kernels(uint32_t) { return sim::setup("setup_conv_kernels"); }
hipError_t launch_conv(uint32_t n, bool, const v2f *src, const v2f *filter, v2f *dst, uint64_t batch, uint64_t filters, float, hipStream_t st)
{
    return sim::launch("launch_conv", st, {Region{src, n * E, {{batch, n * E}}}, Region{filter, n * E, {{filters, n * E}}}},
                       {Region{dst, n * E, {{batch, n * E}}}});
}
}  // namespace fwc
namespace fwt {
hipError_t setup_stft_kernels(uint32_t) { return sim::setup("setup_stft_kernels"); }
// The framed plans, from the prose of kernels_stft.hip and stft_geom.h and none of their functions: `src` holds `signals` signals of
// L f32 back to back, frame f of signal s is the n floats from s L + f hop on, f < F = 1 + (L - n) / hop; frame g = s F + f is row g of
// `dst`, n / 2 + 1 values of 8 bytes (spectrum) or 4 (power), no padding.  A workgroup owns 256 adjacent frames up to n = 64 and 16
// from n = 128 on; the last one owns what is left.  Every workgroup reads the 4 n window bytes when there is a window.
hipError_t launch_stft(uint32_t n, uint32_t hop, uint64_t L, uint64_t signals, bool power, const float *src, const float *window, float *dst,
                       hipStream_t st)
{
    const uint64_t F = 1 + (L - n) / hop, frames = signals * F, per_wg = n <= 64 ? 256 : 16, row = (power ? 4ull : 8ull) * (n / 2 + 1);
    const uint64_t whole = frames / per_wg, rest = frames % per_wg;
    sim::note_grid(whole + (rest != 0));
    std::vector<Region> rd = {Region{src, 4ull * n, {{F, 4ull * hop}, {signals, 4ull * L}}}};
    if (window) rd.push_back(flat(window, n, 4));
    // the rows of one workgroup, workgroup by workgroup: a stride below the length of what it steps over would be two workgroups
    // (or two frames) on the same bytes
    std::vector<Region> wr = {Region{dst, row, {{per_wg, row}, {whole, per_wg * row}}}};
    if (rest) wr.push_back(Region{reinterpret_cast<const char *>(dst) + whole * per_wg * row, row, {{rest, row}}});
    return sim::launch("launch_stft", st, rd, wr);
}
}  // namespace fwt
