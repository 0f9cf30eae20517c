// t1render_bvh.h -- the host-side builder of the robot mesh's bounding volume hierarchies (t1render_mesh_create,
// include/t1render.h).  Plain C++, no HIP: tests/render_bvh_main.cpp compiles and runs it on a CPU.
//
// Input: ntri triangles in the frame of their body (nine floats each: v0, v1, v2), a body in [0, NB) and a colour per
// triangle.  Output: one binary tree per body that has a triangle, all in one node array, and the triangles in leaf
// order, each with its index in the caller's order.  A body's triangles are contiguous (first, count), its nodes too.
//
// The build rule (deterministic: the same input gives the same bytes):
//   * a node of at most LEAF triangles is a leaf;
//   * else the triangles are ordered by their centroid ((v0 + v1 + v2) / 3, in double) along the axis on which the
//     centroids' box is widest (equal widths: the lower axis), equal coordinates by the caller's index; the first
//     ceil(n / 2) go to the left child, the rest to the right.  A child is never empty, so a mesh of identical
//     triangles terminates, and a leaf lies at most max(0, ceil(log2 n) - 2) <= ceil(log2 n) levels below the root;
//   * the two children of a node are neighbours in the node array (left, left + 1); leaves hand out the triangle
//     array front to back, so leaf order is depth-first order.
// ntri > MAX_TRI = 2^20 is refused: no tree is deeper than 18, and the kernel's 24-entry stack cannot overflow.
//
// A triangle is stored as v0 and the edges e1 = v1 - v0, e2 = v2 - v0 (what Moeller-Trumbore reads).  A triangle whose
// cross product (v1 - v0) x (v2 - v0) is zero in double has its edges stored as zero: the kernel's determinant is then
// exactly zero for every ray, and the triangle is never hit.
//
// Boxes.  The kernel accepts a hit only at a point inside the triangle's own box -- the componentwise range of v0,
// fl(v0 + e1), fl(v0 + e2), evaluated in float exactly as here (the builder's box also takes in the caller's v1 and
// v2) -- widened by a margin that grows with the ray's distance (t1render_mesh.hip: tri_hit), and it widens every
// node box it tests by a larger one.  A leaf's box is the
// union of its triangles' boxes, a node's the union of its children's; each is then padded by PAD_ABS + PAD_REL *
// (largest |coordinate|) and stepped one float outward.  So a bound errs only towards visiting: a point at which the
// kernel's intersection routine accepts a hit lies inside every box above its triangle, with room for the slab test's
// own rounding.  radius[b]: no such point of body b is further from the body's origin than radius[b] plus the
// kernel's margin (the farthest corner of any triangle's padded box).
#ifndef T1RENDER_BVH_H
#define T1RENDER_BVH_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace t1bvh {

constexpr int NB = 13;                 // bodies of the collapsed robot
constexpr int LEAF = 4;                // triangles per leaf, at most
constexpr int32_t MAX_TRI = 1 << 20;
constexpr int STACK = 24;              // entries of the kernel's traversal stack
constexpr float PAD_ABS = 1e-6f, PAD_REL = 1e-6f;

struct Node {      // 32 bytes: one read
  float lo[3], hi[3];
  int32_t a, b;    // b == 0: inner, children a and a + 1;  b > 0: leaf, triangles a .. a + b - 1
};
struct Tri {       // 48 bytes: three 16-byte reads
  float v0[3], e1[3], e2[3];
  int32_t idx;     // the caller's index
  uint32_t rgb;
  int32_t body;
};
static_assert(sizeof(Node) == 32 && sizeof(Tri) == 48, "device layout");

struct Mesh {
  std::vector<Node> nodes;
  std::vector<Tri> tris;                       // leaf order; tris.size() == ntri
  int32_t root[NB], first[NB], count[NB];      // root: -1 for a body without triangles
  float radius[NB];                            // 0 for a body without triangles
  int32_t max_depth = 0;                       // the deepest leaf of any tree (a root is at depth 0)
};

enum { OK = 0, E_NULL = 1, E_NTRI = 2, E_BODY = 3, E_FINITE = 4 };

namespace detail {

inline float down(float v) { return std::nextafter(v, -INFINITY); }
inline float up(float v) { return std::nextafter(v, INFINITY); }

struct Builder {
  const float* tri;
  std::vector<double> cen;   // 3 per caller triangle
  std::vector<int32_t> order;
  Mesh* M;

  void tri_box(const Tri& T, float lo[3], float hi[3]) const {
    const float* v = tri + 9 * (size_t)T.idx;
    for (int k = 0; k < 3; ++k) {
      const float a = T.v0[k], b = T.v0[k] + T.e1[k], c = T.v0[k] + T.e2[k];   // float adds, as the kernel's
      // and the caller's own v1, v2: fl(v0 + e1) may differ from v1 by a rounding, and a zero-area triangle's do
      lo[k] = std::min(std::min(a, std::min(b, c)), std::min(v[3 + k], v[6 + k]));
      hi[k] = std::max(std::max(a, std::max(b, c)), std::max(v[3 + k], v[6 + k]));
    }
  }
  static void pad(Node& N) {
    float m = 0.0f;
    for (int k = 0; k < 3; ++k) m = std::max(m, std::max(std::fabs(N.lo[k]), std::fabs(N.hi[k])));
    const float p = PAD_ABS + PAD_REL * m;
    for (int k = 0; k < 3; ++k) {
      N.lo[k] = down(N.lo[k] - p);
      N.hi[k] = up(N.hi[k] + p);
    }
  }

  // the node `at` over order[lo, hi)
  void node(size_t at, int32_t lo, int32_t hi, int depth) {
    const int32_t n = hi - lo;
    Node N = {};
    if (n <= LEAF) {
      N.a = (int32_t)M->tris.size();
      N.b = n;
      for (int k = 0; k < 3; ++k) { N.lo[k] = INFINITY; N.hi[k] = -INFINITY; }
      for (int32_t i = lo; i < hi; ++i) {
        Tri T = make_tri(order[i]);
        float tl[3], th[3];
        tri_box(T, tl, th);
        for (int k = 0; k < 3; ++k) { N.lo[k] = std::min(N.lo[k], tl[k]); N.hi[k] = std::max(N.hi[k], th[k]); }
        M->tris.push_back(T);
      }
      pad(N);
      M->nodes[at] = N;
      M->max_depth = std::max(M->max_depth, depth);
      return;
    }
    double cl[3] = {INFINITY, INFINITY, INFINITY}, ch[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int32_t i = lo; i < hi; ++i)
      for (int k = 0; k < 3; ++k) {
        cl[k] = std::min(cl[k], cen[3 * (size_t)order[i] + k]);
        ch[k] = std::max(ch[k], cen[3 * (size_t)order[i] + k]);
      }
    int ax = 0;
    for (int k = 1; k < 3; ++k)
      if (ch[k] - cl[k] > ch[ax] - cl[ax]) ax = k;
    std::sort(order.begin() + lo, order.begin() + hi, [&](int32_t x, int32_t y) {
      const double a = cen[3 * (size_t)x + ax], b = cen[3 * (size_t)y + ax];
      return a < b || (a == b && x < y);
    });
    const int32_t mid = lo + (n + 1) / 2;
    const size_t c = M->nodes.size();
    M->nodes.resize(c + 2);
    node(c, lo, mid, depth + 1);
    node(c + 1, mid, hi, depth + 1);
    const Node &L = M->nodes[c], &R = M->nodes[c + 1];
    for (int k = 0; k < 3; ++k) { N.lo[k] = std::min(L.lo[k], R.lo[k]); N.hi[k] = std::max(L.hi[k], R.hi[k]); }
    pad(N);
    N.a = (int32_t)c;
    N.b = 0;
    M->nodes[at] = N;
  }

  const uint32_t* rgb;
  const int32_t* body;
  Tri make_tri(int32_t i) const {
    const float* v = tri + 9 * (size_t)i;
    Tri T = {};
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
      T.v0[k] = v[k];
      e1[k] = (double)v[3 + k] - (double)v[k];
      e2[k] = (double)v[6 + k] - (double)v[k];
    }
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const bool flat = cx == 0.0 && cy == 0.0 && cz == 0.0;
    for (int k = 0; k < 3; ++k) {
      T.e1[k] = flat ? 0.0f : (float)e1[k];
      T.e2[k] = flat ? 0.0f : (float)e2[k];
    }
    T.idx = i;
    T.rgb = rgb[i];
    T.body = body[i];
    return T;
  }
};

}  // namespace detail

// Returns OK or the first reason to refuse; *out is complete only on OK.
inline int build(const float* tri, const int32_t* body, const uint32_t* rgb, int32_t ntri, Mesh* out) {
  if (!out) return E_NULL;
  if (ntri < 0 || ntri > MAX_TRI) return E_NTRI;
  if (ntri > 0 && (!tri || !body || !rgb)) return E_NULL;
  for (int32_t i = 0; i < ntri; ++i) {
    if (body[i] < 0 || body[i] >= NB) return E_BODY;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(tri[9 * (size_t)i + k])) return E_FINITE;
  }
  Mesh& M = *out;
  M.nodes.clear();
  M.tris.clear();
  M.tris.reserve(ntri);
  M.max_depth = 0;
  detail::Builder B;
  B.tri = tri;
  B.rgb = rgb;
  B.body = body;
  B.M = &M;
  B.cen.resize(3 * (size_t)ntri);
  for (int32_t i = 0; i < ntri; ++i)
    for (int k = 0; k < 3; ++k) {
      const float* v = tri + 9 * (size_t)i;
      B.cen[3 * (size_t)i + k] = ((double)v[k] + (double)v[3 + k] + (double)v[6 + k]) / 3.0;
    }
  B.order.reserve(ntri);
  for (int b = 0; b < NB; ++b) {
    const int32_t lo = (int32_t)B.order.size();
    for (int32_t i = 0; i < ntri; ++i)
      if (body[i] == b) B.order.push_back(i);
    const int32_t hi = (int32_t)B.order.size();
    M.root[b] = -1;
    M.first[b] = (int32_t)M.tris.size();
    M.count[b] = hi - lo;
    M.radius[b] = 0.0f;
    if (hi == lo) continue;
    M.root[b] = (int32_t)M.nodes.size();
    M.nodes.resize(M.nodes.size() + 1);
    B.node(M.root[b], lo, hi, 0);
    double r2 = 0.0;
    for (int32_t i = M.first[b]; i < M.first[b] + M.count[b]; ++i) {
      Node N = {};
      B.tri_box(M.tris[i], N.lo, N.hi);
      detail::Builder::pad(N);
      double s = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double e = std::max(std::fabs((double)N.lo[k]), std::fabs((double)N.hi[k]));
        s += e * e;
      }
      r2 = std::max(r2, s);
    }
    M.radius[b] = detail::up((float)(std::sqrt(r2) * (1.0 + 1e-6) + 1e-6));
  }
  return OK;
}

}  // namespace t1bvh
#endif
