// Part 3 of include/rgbd_pose_hip.h: the keyframe graph (kernels in rpe_graph.hip; rpe_keyframes_link itself lives with the store's
// matcher in rpe_keyframe_api.hip).  Edges given by the host, the read-back entries, the rows and records of one round for inspection,
// and rpe_keyframes_optimize: per round the corrections (fp64 on the host, 12 floats per keyframe up), ONE launch over every edge, one
// copy of the raw records down through the pinned staging, the records turned into tangent-space blocks, the dense solve
// (rpe_graph_solve, library.cpp) and the left update of every free pose.
#include "rpe_graph.h"
using namespace rpeh;

namespace rpeh {

rpe_graph* graph_of(rpe_context* c) {
  if (!c->graph) c->graph = new rpe_graph();
  return c->graph;
}

// the pair arrays double from 64 Ki pairs (the store's own steps: eight keyframes' worth of keypoints x 2)
int graph_reserve(rpe_context* c, int64_t more) {
  rpe_graph* G = graph_of(c);
  const int64_t need = G->used + more;
  if (need <= G->cap()) return RPE_OK;
  int64_t cap = std::max<int64_t>(G->cap(), 16 * (int64_t)rpe::kMaxKeypoints);
  while (cap < need) cap *= 2;
  const size_t keep = (size_t)G->used * sizeof(int), bytes = (size_t)cap * sizeof(int);
  const DevMem::Grow g[] = {{&G->a, keep, bytes}, {&G->b, keep, bytes}};
  return DevMem::regrow(c, "graph storage", g);
}

void graph_drop_from(rpe_context* c, int first) {
  rpe_graph* G = c->graph;
  if (!G) return;
  while (!G->edges.empty() && G->edges.back().j >= first) G->edges.pop_back();   // ordered by (j, i): they are the tail
  G->used = 0;
  for (const auto& e : G->edges) G->used = std::max<int64_t>(G->used, (int64_t)e.off + e.count);
  G->dirty = true;
}

// the live edges' pairs moved together, in edge order, into fresh arrays of the same size (the dead ranges of replaced edges go)
int graph_compact(rpe_context* c) {
  rpe_graph* G = c->graph;
  if (!G || !G->cap()) return RPE_OK;
  DevBuf<int> q[2];   // swapped in on success, gone with this scope otherwise
  int rc;
  if ((rc = q[0].once(c, G->a.bytes())) || (rc = q[1].once(c, G->b.bytes()))) return rc;
  hipError_t e = hipSuccess;
  int64_t at = 0;
  std::vector<int> off(G->edges.size());
  for (size_t n = 0; n < G->edges.size() && e == hipSuccess; n++) {
    const auto& E = G->edges[n];
    off[n] = (int)at;
    if (!E.count) continue;
    e = hipMemcpyAsync(q[0] + at, G->a + E.off, (size_t)E.count * sizeof(int), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q[1] + at, G->b + E.off, (size_t)E.count * sizeof(int), hipMemcpyDeviceToDevice, c->stream);
    at += E.count;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "graph storage: %s", hipGetErrorString(e));
  G->a = std::move(q[0]); G->b = std::move(q[1]); G->used = at; G->dirty = true;
  for (size_t n = 0; n < G->edges.size(); n++) G->edges[n].off = off[n];
  return RPE_OK;
}

void graph_free(rpe_context* c) {
  delete c->graph;
  c->graph = nullptr;
}

}  // namespace rpeh

namespace {

using Pose = std::array<double, 12>;

int graph_ready(rpe_context* c, const char* who) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!c->graph || c->graph->edges.empty())
    return fail(RPE_ERR_STATE, "%s: the graph has no edge (rpe_keyframes_link, rpe_graph_add_edge_host)", who);
  return RPE_OK;
}

// the edge table and the work areas on the device, sized for the current edges
int graph_device(rpe_context* c) {
  rpe_graph* G = c->graph;
  const int n = (int)G->edges.size();
  int rc;
  if ((rc = G->d_corr.once(c, (size_t)rpe::kMaxKeyframes * rpe::kGraphCorr * sizeof(float)))) return rc;
  int cap = std::max(G->edges_cap(), 64);
  while (cap < n) cap *= 2;
  if (n > G->edges_cap()) G->dirty = true;
  if ((rc = G->d_edges.reserve(c, (size_t)cap * sizeof(rpe::GraphEdgeDev))) ||
      (rc = G->d_raw.reserve(c, (size_t)cap * rpe::kGraphRaw * sizeof(double)))) return rc;
  if (G->dirty) {
    std::vector<rpe::GraphEdgeDev> t(n);
    int out = 0;
    for (int e = 0; e < n; e++) { const auto& E = G->edges[e]; t[e] = rpe::GraphEdgeDev{E.j, E.i, E.off, E.count, out, 0}; out += E.count; }
    HIP_TRY(hipMemcpyAsync(G->d_edges, t.data(), (size_t)n * sizeof(rpe::GraphEdgeDev), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // `t` is the host's again
    G->dirty = false;
  }
  return RPE_OK;
}

void mat3_tmul(const double* A, const double* B, double* out) {      // out = A^T B
  for (int r = 0; r < 3; r++) for (int s = 0; s < 3; s++) out[3 * r + s] = (A[r] * B[s] + A[3 + r] * B[3 + s]) + A[6 + r] * B[6 + s];
}

// the corrections of trial poses P against the store's: C_k = R_k^T R0_k, c_k = R_k^T (t0_k - t_k) in fp64, cast to fp32; a pose that
// IS the store's (the same bits) gives the identity exactly.  Uploaded: 12 floats per keyframe
int upload_corrections(rpe_context* c, const std::vector<Pose>& P) {
  const auto& K = c->kf;
  const int n = (int)K.meta.size();
  std::vector<float> h((size_t)n * rpe::kGraphCorr);
  for (int k = 0; k < n; k++) {
    const double *p = P[k].data(), *p0 = K.meta[k].pose;
    float* o = h.data() + (size_t)k * rpe::kGraphCorr;
    if (std::memcmp(p, p0, sizeof(Pose)) == 0) { for (int m = 0; m < 12; m++) o[m] = (m < 9 && m % 4 == 0) ? 1.f : 0.f; continue; }
    double Cm[9], d[3] = {p0[9] - p[9], p0[10] - p[10], p0[11] - p[11]};
    mat3_tmul(p, p0, Cm);
    for (int m = 0; m < 9; m++) o[m] = (float)Cm[m];
    for (int r = 0; r < 3; r++) o[9 + r] = (float)((p[r] * d[0] + p[3 + r] * d[1]) + p[6 + r] * d[2]);
  }
  HIP_TRY(hipMemcpyAsync(c->graph->d_corr, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPE_OK;
}

float gate_sq(double gate) { const float g = (float)gate; return g * g; }

// M_k = [[R^T, -R^T [t]x], [0, R^T]] (6 x 6, row-major): the world-frame Jacobian A(X) = [-I, [X]x] times M_k is the derivative of
// X_k by the left update (upsilon, omega) of pose k
void tangent_map(const double* p, double* M) {
  const double tx[9] = {0, -p[11], p[10], p[11], 0, -p[9], -p[10], p[9], 0};
  double B[9];
  mat3_tmul(p, tx, B);
  for (int r = 0; r < 6; r++) for (int s = 0; s < 6; s++) M[6 * r + s] = 0.0;
  for (int r = 0; r < 3; r++) for (int s = 0; s < 3; s++) {
    M[6 * r + s] = p[3 * s + r]; M[6 * (r + 3) + s + 3] = p[3 * s + r]; M[6 * r + s + 3] = -B[3 * r + s];
  }
}
void skew_add(double* H, int r0, int c0, const double* v, double sgn) {   // H[r0.., c0..] += sgn [v]x   (H 6 x 6)
  H[6 * r0 + c0 + 1] += -sgn * v[2]; H[6 * r0 + c0 + 2] += sgn * v[1];
  H[6 * (r0 + 1) + c0] += sgn * v[2]; H[6 * (r0 + 1) + c0 + 2] += -sgn * v[0];
  H[6 * (r0 + 2) + c0] += -sgn * v[1]; H[6 * (r0 + 2) + c0 + 1] += sgn * v[0];
}
// world-frame block of one keyframe with itself: [[n I, -[S]x], [[S]x, tr(Q) I - Q]], Q = the 6 second moments
void self_block(double n, const double* S, const double* Q6, double* H) {
  for (int k = 0; k < 36; k++) H[k] = 0.0;
  const double Q[9] = {Q6[0], Q6[1], Q6[2], Q6[1], Q6[3], Q6[4], Q6[2], Q6[4], Q6[5]}, tr = (Q6[0] + Q6[3]) + Q6[5];
  for (int r = 0; r < 3; r++) {
    H[6 * r + r] = n;
    for (int s = 0; s < 3; s++) H[6 * (r + 3) + s + 3] = (r == s ? tr : 0.0) - Q[3 * r + s];
  }
  skew_add(H, 0, 3, S, -1.0);
  skew_add(H, 3, 0, S, 1.0);
}
void congruence(const double* A, const double* H, const double* B, double* out) {   // out = A^T H B, all 6 x 6
  double T[36];
  for (int r = 0; r < 6; r++) for (int s = 0; s < 6; s++) { double v = 0; for (int k = 0; k < 6; k++) v += H[6 * r + k] * B[6 * k + s]; T[6 * r + s] = v; }
  for (int r = 0; r < 6; r++) for (int s = 0; s < 6; s++) { double v = 0; for (int k = 0; k < 6; k++) v += A[6 * k + r] * T[6 * k + s]; out[6 * r + s] = v; }
}
// one raw record (rpe_graph.hip) -> the RPE_GRAPH_RECORD doubles of the header, at the poses pj / pi
void graph_record(const double* w, const double* pj, const double* pi, double* rec) {
  double Mj[36], Mi[36], Hjj[36], Hii[36], Hji[36], T[36];
  tangent_map(pj, Mj); tangent_map(pi, Mi);
  const double gj[6] = {-w[2], -w[3], -w[4], w[5], w[6], w[7]}, gi[6] = {w[2], w[3], w[4], w[8], w[9], w[10]};
  rec[0] = w[0]; rec[1] = w[1];
  for (int r = 0; r < 6; r++) {
    double a = 0, b = 0;
    for (int k = 0; k < 6; k++) { a += Mj[6 * k + r] * gj[k]; b += Mi[6 * k + r] * gi[k]; }
    rec[2 + r] = a; rec[8 + r] = b;
  }
  self_block(w[0], w + 11, w + 17, T); congruence(Mj, T, Mj, Hjj);
  self_block(w[0], w + 14, w + 23, T); congruence(Mi, T, Mi, Hii);
  // the cross block [[-n I, [SY]x], [-[SX]x, (sum X Y^T)^T - tr(sum X Y^T) I]]
  for (int k = 0; k < 36; k++) T[k] = 0.0;
  const double tr = (w[29] + w[33]) + w[37];
  for (int r = 0; r < 3; r++) {
    T[6 * r + r] = -w[0];
    for (int s = 0; s < 3; s++) T[6 * (r + 3) + s + 3] = w[29 + 3 * s + r] - (r == s ? tr : 0.0);
  }
  skew_add(T, 0, 3, w + 14, 1.0);
  skew_add(T, 3, 0, w + 11, -1.0);
  congruence(Mj, T, Mi, Hji);
  int k = 14;
  for (int r = 0; r < 6; r++) for (int s = r; s < 6; s++) rec[k++] = Hjj[6 * r + s];
  for (int r = 0; r < 6; r++) for (int s = r; s < 6; s++) rec[k++] = Hii[6 * r + s];
  for (int m = 0; m < 36; m++) rec[k++] = Hji[m];
}

int poses_of(rpe_context* c, const double* poses12, std::vector<Pose>* P) {
  const auto& K = c->kf;
  P->resize(K.meta.size());
  for (size_t k = 0; k < K.meta.size(); k++) std::memcpy((*P)[k].data(), poses12 ? poses12 + 12 * k : K.meta[k].pose, sizeof(Pose));
  for (const Pose& p : *P) for (double v : p) if (!std::isfinite(v)) return fail(RPE_ERR_ARG, "a pose is not finite");
  return RPE_OK;
}

// one round at the poses P: corrections up, the launch, the raw records down, the records of the header in rec (edges x RPE_GRAPH_RECORD)
int graph_round(rpe_context* c, const std::vector<Pose>& P, double gate, std::vector<double>* raw, double* rec) {
  rpe_graph* G = c->graph;
  const int n = (int)G->edges.size();
  int rc;
  if ((rc = upload_corrections(c, P))) return rc;
  HIP_TRY(rpe::launch_graph_round(G->d_edges, n, G->a, G->b, c->kf.store(), G->d_corr, gate_sq(gate), G->d_raw, c->stream));
  raw->resize((size_t)n * rpe::kGraphRaw);
  if ((rc = copy_to_host(c, raw->data(), G->d_raw, raw->size() * sizeof(double)))) return rc;
  for (int e = 0; e < n; e++)
    graph_record(raw->data() + (size_t)e * rpe::kGraphRaw, P[G->edges[e].j].data(), P[G->edges[e].i].data(), rec + (size_t)e * RPE_GRAPH_RECORD);
  return RPE_OK;
}

}  // namespace

extern "C" {

int rpe_graph_add_edge_host(rpe_context* c, int j, int i, int count, const int32_t* a, const int32_t* b) {
  session_end(c);
  if (!c || !a || !b || count < 1 || count > RPE_MAX_KEYPOINTS)
    return fail(RPE_ERR_ARG, "rpe_graph_add_edge_host: bad argument (count 1 .. %d, a and b not NULL)", RPE_MAX_KEYPOINTS);
  const int n = (int)c->kf.meta.size();
  if (j <= i || i < 0 || j >= n) return fail(RPE_ERR_ARG, "rpe_graph_add_edge_host: edge (%d, %d) needs 0 <= i < j < %d keyframes", j, i, n);
  const int nj = c->kf.meta[j].count, ni = c->kf.meta[i].count;
  for (int k = 0; k < count; k++)
    if (a[k] < 0 || a[k] >= nj || b[k] < 0 || b[k] >= ni)
      return fail(RPE_ERR_ARG, "rpe_graph_add_edge_host: pair %d = (%d, %d) is outside the keyframes (%d and %d keypoints)", k, a[k], b[k], nj, ni);
  HIP_TRY(hipSetDevice(c->device));
  rpe_graph* G = graph_of(c);
  const rpe_graph::Edge key{j, i, 0, 0};
  auto it = std::lower_bound(G->edges.begin(), G->edges.end(), key,
                             [](const rpe_graph::Edge& x, const rpe_graph::Edge& y) { return x.j != y.j ? x.j < y.j : x.i < y.i; });
  const bool replace = it != G->edges.end() && it->j == j && it->i == i;
  int rc, off;
  if (replace && count <= it->count) off = it->off;            // the new pairs fit where the old ones are
  else {
    // behind the last live edge.  A replaced edge's old pairs are dead until then: once the dead outweigh the live, the live ones
    // are moved together first, so replacing edges again and again does not grow the arrays
    const size_t at = (size_t)(it - G->edges.begin());
    if (replace) it->count = 0;
    if (G->used > 2 * (G->pairs() + count) && (rc = graph_compact(c))) return rc;
    if (G->used + count > kGraphMaxPairs) return fail(RPE_ERR_STATE, "rpe_graph_add_edge_host: more than 2^30 pairs");
    if ((rc = graph_reserve(c, count))) return rc;
    it = G->edges.begin() + at;
    off = (int)G->used;
    G->used += count;
  }
  HIP_TRY(hipMemcpyAsync(G->a + off, a, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(G->b + off, b, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const rpe_graph::Edge E{j, i, off, count};
  if (replace) *it = E; else G->edges.insert(it, E);
  G->dirty = true;
  return RPE_OK;
}

int rpe_graph_info(rpe_context* c, int* edges, int64_t* pairs) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (edges) *edges = c->graph ? (int)c->graph->edges.size() : 0;
  if (pairs) *pairs = c->graph ? c->graph->pairs() : 0;
  return RPE_OK;
}

int rpe_graph_edges(rpe_context* c, int32_t* jic) {
  if (!c) return fail(RPE_ERR_ARG, "null context");
  if (!c->graph || c->graph->edges.empty()) return RPE_OK;
  if (!jic) return fail(RPE_ERR_ARG, "rpe_graph_edges: jic must not be NULL");
  int k = 0;
  for (const auto& e : c->graph->edges) { jic[k++] = e.j; jic[k++] = e.i; jic[k++] = e.count; }
  return RPE_OK;
}

int rpe_graph_edge_download(rpe_context* c, int edge, int32_t* a, int32_t* b) {
  session_end(c);
  if (!c) return fail(RPE_ERR_ARG, "null context");
  const int n = c->graph ? (int)c->graph->edges.size() : 0;
  if (edge < 0 || edge >= n) return fail(RPE_ERR_ARG, "rpe_graph_edge_download: no edge %d (%d in the graph)", edge, n);
  HIP_TRY(hipSetDevice(c->device));
  const auto& E = c->graph->edges[edge];
  int rc;
  if (a && (rc = copy_to_host(c, a, c->graph->a + E.off, (size_t)E.count * sizeof(int)))) return rc;
  if (b && (rc = copy_to_host(c, b, c->graph->b + E.off, (size_t)E.count * sizeof(int)))) return rc;
  return RPE_OK;
}

int rpe_graph_residuals(rpe_context* c, const double* poses12, double gate, float* r) {
  session_end(c);
  int rc = graph_ready(c, "rpe_graph_residuals");
  if (rc) return rc;
  if (!r || !(gate >= 0)) return fail(RPE_ERR_ARG, "rpe_graph_residuals: bad argument (gate >= 0, r not NULL)");
  std::vector<Pose> P;
  if ((rc = poses_of(c, poses12, &P))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = graph_device(c)) || (rc = upload_corrections(c, P))) return rc;
  rpe_graph* G = c->graph;
  const size_t bytes = (size_t)G->pairs() * 3 * sizeof(float);
  DevBuf<float> d_rows;
  if ((rc = d_rows.once(c, bytes))) return rc;
  hipError_t e = rpe::launch_graph_rows(G->d_edges, (int)G->edges.size(), G->a, G->b, c->kf.store(), G->d_corr, gate_sq(gate), d_rows, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(r, d_rows, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RPE_ERR_HIP, "rpe_graph_residuals: %s", hipGetErrorString(e));
  return RPE_OK;
}

int rpe_graph_normal_eq(rpe_context* c, const double* poses12, double gate, double* records) {
  session_end(c);
  int rc = graph_ready(c, "rpe_graph_normal_eq");
  if (rc) return rc;
  if (!records || !(gate >= 0)) return fail(RPE_ERR_ARG, "rpe_graph_normal_eq: bad argument (gate >= 0, records not NULL)");
  std::vector<Pose> P;
  if ((rc = poses_of(c, poses12, &P))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = graph_device(c))) return rc;
  std::vector<double> raw;
  return graph_round(c, P, gate, &raw, records);
}

int rpe_keyframes_optimize(rpe_context* c, int anchor, int rounds, const double* gates, double tol, int apply, double* poses12_out,
                           double* stats, int* rounds_out) {
  session_end(c);
  int rc = graph_ready(c, "rpe_keyframes_optimize");
  if (rc) return rc;
  auto& K = c->kf;
  const int n = (int)K.meta.size();
  if (anchor < 0 || anchor >= n || rounds < 1 || !gates || !(tol >= 0))
    return fail(RPE_ERR_ARG, "rpe_keyframes_optimize: bad argument (anchor one of the %d keyframes, rounds >= 1, gates not NULL, tol >= 0)", n);
  for (int r = 0; r < rounds; r++) if (!(gates[r] >= 0)) return fail(RPE_ERR_ARG, "rpe_keyframes_optimize: bad gate in round %d", r);
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = graph_device(c))) return rc;
  rpe_graph* G = c->graph;
  const int ne = (int)G->edges.size();
  std::vector<Pose> P;
  if ((rc = poses_of(c, nullptr, &P))) return rc;
  std::vector<double> raw, rec((size_t)ne * RPE_GRAPH_RECORD), delta((size_t)6 * n);
  std::vector<int32_t> ji((size_t)2 * ne);
  for (int e = 0; e < ne; e++) { ji[2 * e] = G->edges[e].j; ji[2 * e + 1] = G->edges[e].i; }
  std::vector<uint8_t> fixed(n, 0);
  int done = 0;
  for (int r = 0; r < rounds; r++) {
    if ((rc = graph_round(c, P, gates[r], &raw, rec.data()))) return rc;
    if (r == 0) {
      // components over the edges that count in the first round (ids only decrease along parents): the anchor and the lowest id of
      // every other component stay where they are -- a keyframe without a counted edge is its own component
      std::vector<int> root(n);
      for (int k = 0; k < n; k++) root[k] = k;
      auto find = [&](int k) { while (root[k] != k) k = root[k] = root[root[k]]; return k; };
      for (int e = 0; e < ne; e++)
        if (rec[(size_t)e * RPE_GRAPH_RECORD] >= 1.0) {
          const int x = find(G->edges[e].j), y = find(G->edges[e].i);
          if (x != y) root[std::max(x, y)] = std::min(x, y);
        }
      const int ra = find(anchor);
      for (int k = 0; k < n; k++) { const int q = find(k); fixed[k] = (q == ra) ? (k == anchor) : (k == q); }
    }
    double pairs = 0, cost = 0;
    for (int e = 0; e < ne; e++) { pairs += rec[(size_t)e * RPE_GRAPH_RECORD]; cost += rec[(size_t)e * RPE_GRAPH_RECORD + 1]; }
    if ((rc = rpe_graph_solve(n, ne, ji.data(), rec.data(), fixed.data(), delta.data()))) return rc;   // degenerate: nothing was changed
    double step = 0;
    for (double v : delta) step += v * v;
    step = std::sqrt(step);
    for (int k = 0; k < n; k++) if (!fixed[k]) rpe::se3_left_update(delta.data() + 6 * k, P[k].data());
    if (stats) { stats[3 * r] = pairs; stats[3 * r + 1] = cost; stats[3 * r + 2] = step; }
    done = r + 1;
    if (step < tol) break;
  }
  if (rounds_out) *rounds_out = done;
  if (poses12_out) for (int k = 0; k < n; k++) std::memcpy(poses12_out + 12 * k, P[k].data(), sizeof(Pose));
  if (apply) {
    if ((rc = upload_corrections(c, P))) return rc;
    HIP_TRY(rpe::launch_graph_apply(K.store(), n, (int)K.used, G->d_corr, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; k++) std::memcpy(K.meta[k].pose, P[k].data(), sizeof(Pose));
    if (c->fe.match_kf >= 0) { c->fe.matches = -1; c->fe.match_kf = -1; }   // a keyframe match list's slots held the old points
  }
  return RPE_OK;
}

}  // extern "C"
