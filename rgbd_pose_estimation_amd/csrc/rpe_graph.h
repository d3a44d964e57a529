// The keyframe graph beside the store (rpe_graph_api.hip; kernels in rpe_graph.hip): what the host keeps of it and the few helpers
// the store's unit (rpe_keyframe_api.hip: rpe_keyframes_link, rpe_keyframes_clear) and rpe_destroy need.
#pragma once
#include "rpe_frontend_host.hpp"
#include <array>

struct rpe_graph {
  struct Edge { int j, i, off, count; };   // j > i; `count` pairs from `off` of a / b
  std::vector<Edge> edges;                 // ordered by (j, i)
  int64_t used = 0;                        // pairs in a / b: the end of the last live edge
  rpeh::DevBuf<int> a, b;                  // device: positions inside keyframe j / keyframe i, room for cap() pairs (grown in steps)
  int64_t cap() const { return (int64_t)(a.bytes() / sizeof(int)); }
  rpeh::DevBuf<rpe::GraphEdgeDev> d_edges; // device copy of the edge table (room for edges_cap() edges), uploaded when `dirty`
  int edges_cap() const { return (int)(d_edges.bytes() / sizeof(rpe::GraphEdgeDev)); }
  bool dirty = true;
  rpeh::DevBuf<double> d_raw;              // edges_cap() x kGraphRaw doubles
  rpeh::DevBuf<float> d_corr;              // RPE_MAX_KEYFRAMES x kGraphCorr floats
  int64_t pairs() const { int64_t n = 0; for (const Edge& e : edges) n += e.count; return n; }
};

namespace rpeh __attribute__((visibility("hidden"))) {
rpe_graph* graph_of(rpe_context* c);                       // the context's graph, made on first use
int graph_reserve(rpe_context* c, int64_t more);          // room for `more` pairs behind `used`
constexpr int64_t kGraphMaxPairs = (int64_t)1 << 30;      // offsets into the pair arrays are ints
int graph_compact(rpe_context* c);                        // the live pairs moved together (dead ranges of replaced edges go)
void graph_drop_from(rpe_context* c, int first);          // forget the edges whose newer keyframe is >= first
void graph_free(rpe_context* c);                          // (rpe_destroy)
}  // namespace rpeh
