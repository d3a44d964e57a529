// Probe of the volume's shared device rules (csrc/rpe_volume_field.hpp), one rule per run: volume_rules_probe <rule> <in.bin> <out.bin>.
// The input is a flat table of cases written by tests/test_gpu_volume_rules.py (little-endian, no header: the case count is the file
// size over the record size); one kernel runs one thread per case -- one workgroup per case for the brick rule --, each calling the
// header's function, and the raw outputs are written back.  Nothing of the header is restated here: the probe is compiled with the
// options the library's kernel units take, so it sees each rule as the kernels do.
//
//   rule        case record                                                  output record
//   cull        float lo[3], hi[3]; Camera; PoseF                            int: box_can_update
//   brick       VolumeGeometry; int i0[3], n[3]; Camera; PoseF               int count, rebuild, map: the brick's voxels (inside the volume) for
//                                                                            which voxel_project<1, 0> holds over an all-valid depth plane far
//                                                                            away; box_can_update on the box as volume_fuse_kernel forms it
//                                                                            (min(i0 + n, dim) - 1) and as map_fuse_kernel does (i0 + 7)
//   half        uint32 bits of an fp32                                       65536 x uint32 bits of h2f(pattern), then f2h per case
//   blend       uint rg, bw, o; float W                                      uint rg, bw
//   quantise    float                                                        uint
//   cell        VolumeGeometry; float p[3]                                   int known, i0[3]; float a[3]   (zeros where unknown)
//   brick_word  int wnb[3], wdim0, wdim1, capacity; int s, x, y, z           int ok, pooled; int64 w        (w = 0 where not ok)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rpe_volume_field.hpp"

using namespace rpe;

#define HIP_OK(call)                                                                                        \
  do {                                                                                                      \
    const hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                                 \
      std::fprintf(stderr, "volume_rules_probe: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      std::exit(2);                                                                                         \
    }                                                                                                       \
  } while (0)

namespace {

constexpr int kProbeBlock = 256;
constexpr float kFarDepth = 1e30f;

struct CullCase { float lo[3], hi[3]; Camera cam; PoseF T; };
struct BrickCase { VolumeGeometry G; int i0[3], n[3]; Camera cam; PoseF T; };
struct BrickOut { int count, rebuild, map; };
struct BlendCase { unsigned rg, bw, o; float W; };
struct BlendOut { unsigned rg, bw; };
struct CellCase { VolumeGeometry G; float p[3]; };
struct CellOut { int known, i0[3]; float a[3]; };
struct WordView { int wnb[3], wdim0, wdim1, capacity; };
struct WordCase { WordView M; int s, x, y, z; };
struct WordOut { int ok, pooled; long long w; };
static_assert(sizeof(CullCase) == 96 && sizeof(BrickCase) == 132 && sizeof(BrickOut) == 12 && sizeof(BlendCase) == 16, "record layout");
static_assert(sizeof(CellCase) == 48 && sizeof(CellOut) == 28 && sizeof(WordCase) == 40 && sizeof(WordOut) == 16, "record layout");

__global__ __launch_bounds__(kProbeBlock) void cull_kernel(const CullCase* in, int* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c >= n) return;
  const CullCase C = in[c];
  out[c] = box_can_update(C.lo, C.hi, C.cam, C.T) ? 1 : 0;
}

__global__ __launch_bounds__(kProbeBlock) void brick_kernel(const BrickCase* in, const float* plane, BrickOut* out) {
  __shared__ int total;
  const BrickCase C = in[blockIdx.x];
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int mine = 0;
  const int nv = C.n[0] * C.n[1] * C.n[2];
  for (int v = threadIdx.x; v < nv; v += kProbeBlock) {
    const int i = C.i0[0] + v % C.n[0], j = C.i0[1] + (v / C.n[0]) % C.n[1], k = C.i0[2] + v / (C.n[0] * C.n[1]);
    if (i >= C.G.dim[0] || j >= C.G.dim[1] || k >= C.G.dim[2]) continue;
    float f, sdf;
    int64_t pix;
    if (voxel_project<1, 0>(C.G, plane, C.cam, C.T, i, j, k, f, sdf, pix)) mine++;
  }
  atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const VolumeGeometry& G = C.G;
  float lo[3], hr[3], hm[3];
  for (int a = 0; a < 3; a++) {
    const int last = min(C.i0[a] + C.n[a], G.dim[a]) - 1;
    lo[a] = G.o[a] + ((float)C.i0[a] + 0.5f) * G.s;
    hr[a] = G.o[a] + ((float)last + 0.5f) * G.s;
    hm[a] = G.o[a] + ((float)(C.i0[a] + 7) + 0.5f) * G.s;
  }
  BrickOut o;
  o.count = total;
  o.rebuild = box_can_update(lo, hr, C.cam, C.T) ? 1 : 0;
  o.map = box_can_update(lo, hm, C.cam, C.T) ? 1 : 0;
  out[blockIdx.x] = o;
}

// out[0 .. 65535] = the bits of h2f(pattern); out[65536 + c] = f2h of case c
__global__ __launch_bounds__(kProbeBlock) void half_kernel(const unsigned* in, unsigned* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c < 65536) out[c] = __float_as_uint(h2f((unsigned)c));
  if (c < n) out[65536 + c] = f2h(__uint_as_float(in[c]));
}

__global__ __launch_bounds__(kProbeBlock) void blend_kernel(const BlendCase* in, BlendOut* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c >= n) return;
  BlendOut o{in[c].rg, in[c].bw};
  blend(o.rg, o.bw, in[c].o, in[c].W);
  out[c] = o;
}

__global__ __launch_bounds__(kProbeBlock) void quantise_kernel(const float* in, unsigned* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c < n) out[c] = quantise(in[c]);
}

__global__ __launch_bounds__(kProbeBlock) void cell_kernel(const CellCase* in, CellOut* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c >= n) return;
  const CellCase C = in[c];
  int i0[3] = {0, 0, 0};
  float a[3] = {0.0f, 0.0f, 0.0f};
  CellOut o{};
  if (cell(C.G, C.p[0], C.p[1], C.p[2], i0, a)) {
    o.known = 1;
    for (int d = 0; d < 3; d++) { o.i0[d] = i0[d]; o.a[d] = a[d]; }
  }
  out[c] = o;
}

__global__ __launch_bounds__(kProbeBlock) void word_kernel(const WordCase* in, WordOut* out, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (c >= n) return;
  const WordCase C = in[c];
  int64_t w = 0;
  bool pooled = false;
  WordOut o{};
  if (brick_word(C.M, C.s, C.x, C.y, C.z, w, pooled)) { o.ok = 1; o.w = w; }
  o.pooled = pooled ? 1 : 0;
  out[c] = o;
}

std::vector<char> read_file(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "volume_rules_probe: cannot read %s\n", path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long size = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> data((size_t)size);
  if (size > 0 && std::fread(data.data(), 1, (size_t)size, f) != (size_t)size) { std::fprintf(stderr, "volume_rules_probe: short read of %s\n", path); std::exit(2); }
  std::fclose(f);
  return data;
}

void write_file(const char* path, const std::vector<char>& data) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(data.data(), 1, data.size(), f) != data.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "volume_rules_probe: cannot write %s\n", path);
    std::exit(2);
  }
}

void bad(const char* what, int64_t c) {
  std::fprintf(stderr, "volume_rules_probe: case %lld: %s\n", (long long)c, what);
  std::exit(2);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: volume_rules_probe <rule> <in.bin> <out.bin>\n"); return 2; }
  const std::string rule = argv[1];
  const std::vector<char> in = read_file(argv[2]);
  size_t rec = 0, orec = 0, extra = 0;
  if (rule == "cull") { rec = sizeof(CullCase); orec = sizeof(int); }
  else if (rule == "brick") { rec = sizeof(BrickCase); orec = sizeof(BrickOut); }
  else if (rule == "half") { rec = sizeof(unsigned); orec = sizeof(unsigned); extra = 65536 * sizeof(unsigned); }
  else if (rule == "blend") { rec = sizeof(BlendCase); orec = sizeof(BlendOut); }
  else if (rule == "quantise") { rec = sizeof(float); orec = sizeof(unsigned); }
  else if (rule == "cell") { rec = sizeof(CellCase); orec = sizeof(CellOut); }
  else if (rule == "brick_word") { rec = sizeof(WordCase); orec = sizeof(WordOut); }
  else { std::fprintf(stderr, "volume_rules_probe: unknown rule %s\n", rule.c_str()); return 2; }
  if (in.size() % rec != 0 || in.size() / rec > ((size_t)1 << 26)) { std::fprintf(stderr, "volume_rules_probe: %zu bytes are no table of %zu-byte cases\n", in.size(), rec); return 2; }
  const int64_t n = (int64_t)(in.size() / rec);

  // the one rule that reads memory through its case: the pixel index stays inside the plane, the voxel loop is bounded
  int64_t plane_px = 0;
  if (rule == "brick") {
    const BrickCase* C = reinterpret_cast<const BrickCase*>(in.data());
    for (int64_t c = 0; c < n; c++) {
      if (C[c].cam.width < 1 || C[c].cam.height < 1 || (int64_t)C[c].cam.width * C[c].cam.height > (1 << 20)) bad("image size", c);
      for (int a = 0; a < 3; a++)
        if (C[c].n[a] < 1 || C[c].n[a] > 64 || C[c].G.dim[a] < 1 || C[c].G.dim[a] > 1024 || C[c].i0[a] < 0 || C[c].i0[a] >= C[c].G.dim[a]) bad("brick", c);
      plane_px = std::max(plane_px, (int64_t)C[c].cam.width * C[c].cam.height);
    }
  }

  const size_t out_bytes = extra + (size_t)n * orec;
  char *d_in = nullptr, *d_out = nullptr;
  float* d_plane = nullptr;
  HIP_OK(hipMalloc(&d_in, std::max<size_t>(in.size(), 16)));
  HIP_OK(hipMalloc(&d_out, std::max<size_t>(out_bytes, 16)));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0, std::max<size_t>(out_bytes, 16)));
  if (plane_px > 0) {
    const std::vector<float> plane((size_t)plane_px, kFarDepth);
    HIP_OK(hipMalloc(&d_plane, plane.size() * sizeof(float)));
    HIP_OK(hipMemcpy(d_plane, plane.data(), plane.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const unsigned grid = (unsigned)((std::max<int64_t>(n, rule == "half" ? 65536 : 1) + kProbeBlock - 1) / kProbeBlock);
  if (rule == "cull") cull_kernel<<<grid, kProbeBlock>>>((const CullCase*)d_in, (int*)d_out, n);
  else if (rule == "brick") { if (n > 0) brick_kernel<<<(unsigned)n, kProbeBlock>>>((const BrickCase*)d_in, d_plane, (BrickOut*)d_out); }
  else if (rule == "half") half_kernel<<<grid, kProbeBlock>>>((const unsigned*)d_in, (unsigned*)d_out, n);
  else if (rule == "blend") blend_kernel<<<grid, kProbeBlock>>>((const BlendCase*)d_in, (BlendOut*)d_out, n);
  else if (rule == "quantise") quantise_kernel<<<grid, kProbeBlock>>>((const float*)d_in, (unsigned*)d_out, n);
  else if (rule == "cell") cell_kernel<<<grid, kProbeBlock>>>((const CellCase*)d_in, (CellOut*)d_out, n);
  else word_kernel<<<grid, kProbeBlock>>>((const WordCase*)d_in, (WordOut*)d_out, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<char> out(out_bytes);
  HIP_OK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));
  if (d_plane) HIP_OK(hipFree(d_plane));
  write_file(argv[3], out);
  std::printf("volume_rules_probe: %s: %lld cases\n", rule.c_str(), (long long)n);
  return 0;
}
