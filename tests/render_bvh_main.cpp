// render_bvh_main.cpp -- a stand-alone driver of csrc/t1render_bvh.h for tests/test_render_bvh_host.py (no HIP, no
// device): reads a mesh, builds it twice, and writes the build for the test to examine.
//   in:  int32 ntri, float tri[9 ntri], int32 body[ntri], uint32 rgb[ntri]
//   out: int32 status, same (the second build's bytes equal the first's), nnodes, ntri, max_depth,
//        int32 root[13], first[13], count[13], float radius[13], Node nodes[nnodes], Tri tris[ntri]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ti5_isaacgym_amd/csrc/t1render_bvh.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static bool same(const t1bvh::Mesh& a, const t1bvh::Mesh& b) {
  return a.nodes.size() == b.nodes.size() && a.tris.size() == b.tris.size() && a.max_depth == b.max_depth &&
         (a.nodes.empty() || !memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(t1bvh::Node))) &&
         (a.tris.empty() || !memcmp(a.tris.data(), b.tris.data(), a.tris.size() * sizeof(t1bvh::Tri))) &&
         !memcmp(a.root, b.root, sizeof a.root) && !memcmp(a.first, b.first, sizeof a.first) &&
         !memcmp(a.count, b.count, sizeof a.count) && !memcmp(a.radius, b.radius, sizeof a.radius);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ntri = 0;
  std::vector<float> tri;
  std::vector<int32_t> body;
  std::vector<uint32_t> rgb;
  const bool ok = fread(&ntri, 4, 1, f) == 1 && ntri >= 0 && read_n(f, tri, 9 * (size_t)ntri) &&
                  read_n(f, body, (size_t)ntri) && read_n(f, rgb, (size_t)ntri);
  fclose(f);
  if (!ok) return 2;
  // a vector of size 0 may hand out a null pointer, which build() refuses only when there is something to read
  static const float none_f = 0.0f;
  static const int32_t none_i = 0;
  static const uint32_t none_u = 0;
  const float* tp = ntri ? tri.data() : &none_f;
  const int32_t* bp = ntri ? body.data() : &none_i;
  const uint32_t* cp = ntri ? rgb.data() : &none_u;
  t1bvh::Mesh a, b;
  const int32_t status = t1bvh::build(tp, bp, cp, ntri, &a);
  const int32_t again = t1bvh::build(tp, bp, cp, ntri, &b);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t head[5] = {status, status == again && (status != t1bvh::OK || same(a, b)) ? 1 : 0,
                           (int32_t)a.nodes.size(), (int32_t)a.tris.size(), a.max_depth};
  fwrite(head, 4, 5, o);
  if (status == t1bvh::OK) {
    fwrite(a.root, 4, t1bvh::NB, o);
    fwrite(a.first, 4, t1bvh::NB, o);
    fwrite(a.count, 4, t1bvh::NB, o);
    fwrite(a.radius, 4, t1bvh::NB, o);
    if (!a.nodes.empty()) fwrite(a.nodes.data(), sizeof(t1bvh::Node), a.nodes.size(), o);
    if (!a.tris.empty()) fwrite(a.tris.data(), sizeof(t1bvh::Tri), a.tris.size(), o);
  }
  fclose(o);
  return 0;
}
