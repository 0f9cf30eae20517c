// t1render_mesh.hip -- t1render_mesh_* (include/t1render.h): the headless camera with the robot drawn as its visual
// meshes, some 48k triangles per robot, through one bounding volume hierarchy per body (t1render_bvh.h builds them on
// the host at create; nodes and leaf-ordered triangles then live in device memory and, a few MB, in L2).
//
//   k_mesh_bounds   one lane per env: the padded sphere around the balls (body origin, radius[b] of the create) of the
//                   posed bodies that carry triangles, and the lowest sphere bottom -- k_scene_bounds with the mesh's
//                   extents in place of the primitives';
//   k_scene_bits    t1render_scene_dev.h, as t1render_scene runs it;
//   k_mesh          16 x 16 pixel workgroups.  The tile-level scan of t1render_scene_dev.h hands out the surviving envs
//                   in env order; BATCH_ENVS of them at a time have their 13 body frames posed into LDS.  A pixel takes its
//                   ray into the frame of each body (o' = R^T (o - p), d' = R^T d: the ray's parameter t is kept),
//                   rejects the body by its root box and walks its tree: both children are slab-tested against the
//                   current best t, the nearer is entered first, the other pushed.  The shadow ray walks the same way
//                   and stops at the first blocker.  Without OTHERS the scan hands out the camera's env alone.
//
// The stack is 24 entries per lane in LDS (24 KiB), entry k of lane l at word 256 k + l: lane l only ever touches bank
// l mod 64, so the lanes of a wave never conflict, whatever their depths.  No run-time-indexed register array, no
// scratch.  t1render_bvh.h bounds the depth at 18.
//
// Soundness of the pruning.  tri_hit accepts a hit at t only when the point fl(o' + t d') lies in the triangle's own
// box widened by m = TRI_MARGIN s, with s = |o'|_1 + radius[b]: the scale of every rounding involved.  Every node box
// above the triangle contains that box (the builder), and box_near widens the node box by M = BOX_MARGIN s before its
// slab test.  M - m = 1e-5 s is more than forty times the rounding of the slab arithmetic (a handful of operations on
// values of magnitude at most 2 s, 6e-8 relative each), so the slab interval computed for a box above an accepted hit
// contains that hit's t, and a node is skipped only when that interval misses (tlo, best].  T1RENDER_MESH_BRUTE tests
// every triangle of a body whose root box is entered, through the same tri_hit on the same operands; both paths keep
// the smallest (t, env, caller's index), which does not depend on the order of the tests: their planes are equal to
// the bit.  The margin costs a grazing hit whose t is off by more than m along the ray (an angle to the triangle's
// plane below about 0.3 degrees), where the pixel is a silhouette pixel anyway.
#include <mutex>
#include <set>

#include "t1render_bvh.h"
#include "t1render_scene_dev.h"

struct t1render_mesh {
  float4* nodes;
  float4* tris;
  int32_t ntri, nnodes, max_depth;
  int32_t root[t1bvh::NB], first[t1bvh::NB], count[t1bvh::NB];
  float radius[t1bvh::NB];
};

namespace {

constexpr int NB = t1bvh::NB;
constexpr int BATCH_ENVS = 8;   // envs posed into LDS at a time
constexpr int STACK = t1bvh::STACK;
constexpr float TRI_MARGIN = 1e-5f, BOX_MARGIN = 2e-5f;
constexpr int FLAGS_ALL = T1RENDER_SCENE_OTHERS | T1RENDER_SCENE_TERRAIN_SHADOW | T1RENDER_SCENE_BRUTE | T1RENDER_MESH_BRUTE;
static_assert(BATCH_ENVS * NB <= CHUNK, "one lane poses one body of a batch");

struct MeshDev {
  const float4* nodes;   // 2 per node (t1bvh::Node)
  const float4* tris;    // 3 per triangle (t1bvh::Tri)
  int32_t root[NB], first[NB], count[NB];
  float radius[NB];
};
struct MeshArgs {
  SceneArgs S;   // S.R.nprims: 1 when the mesh has a triangle, else 0 (what k_scene_bits calls a live env)
  MeshDev M;
  int32_t* tris_out;
};

struct BodyFrame {
  float p[3], R[9];   // origin and body-to-world rotation (row major)
};
struct Batch {
  BodyFrame body[BATCH_ENVS * NB];
  int32_t env[BATCH_ENVS];
  int32_t stack[STACK * CHUNK];
  Scan scan;
  Frame cam;
};

// the frame of one body from its rigid_state row: the arithmetic of pose_scene (t1render.hip)
__device__ __forceinline__ void pose_body(BodyFrame& B, const float* b) {
  const float x = b[3], y = b[4], z = b[5], w = b[6];
  B.p[0] = b[0]; B.p[1] = b[1]; B.p[2] = b[2];
  B.R[0] = 1 - 2 * (y * y + z * z); B.R[1] = 2 * (x * y - z * w);     B.R[2] = 2 * (x * z + y * w);
  B.R[3] = 2 * (x * y + z * w);     B.R[4] = 1 - 2 * (x * x + z * z); B.R[5] = 2 * (y * z - x * w);
  B.R[6] = 2 * (x * z - y * w);     B.R[7] = 2 * (y * z + x * w);     B.R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ F3 to_body(const BodyFrame& B, F3 v) {   // R^T v
  return f3(B.R[0] * v.x + B.R[3] * v.y + B.R[6] * v.z, B.R[1] * v.x + B.R[4] * v.y + B.R[7] * v.z,
            B.R[2] * v.x + B.R[5] * v.y + B.R[8] * v.z);
}
__device__ __forceinline__ F3 to_world(const BodyFrame& B, F3 v) {   // R v
  return f3(B.R[0] * v.x + B.R[1] * v.y + B.R[2] * v.z, B.R[3] * v.x + B.R[4] * v.y + B.R[5] * v.z,
            B.R[6] * v.x + B.R[7] * v.y + B.R[8] * v.z);
}

__global__ __launch_bounds__(CHUNK) void k_mesh_bounds(const MeshArgs A) {
  const int n = blockIdx.x * CHUNK + threadIdx.x;
  const SceneArgs& S = A.S;
  uint32_t key = 0xffffffffu;
  if (n < S.num_envs) {
    const float* rs = S.R.rigid_state + (size_t)n * 169;
    F3 lo = f3(INFINITY, INFINITY, INFINITY), hi = f3(-INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (A.M.root[b] < 0) continue;
      const float r = A.M.radius[b];
      const F3 p = f3(rs[13 * b], rs[13 * b + 1], rs[13 * b + 2]);
      lo = f3(fminf(lo.x, p.x - r), fminf(lo.y, p.y - r), fminf(lo.z, p.z - r));
      hi = f3(fmaxf(hi.x, p.x + r), fmaxf(hi.y, p.y + r), fmaxf(hi.z, p.z + r));
    }
    // the sphere around the balls' bounding box, padded as k_scene_bounds pads (a quaternion is a unit one to fp32
    // only, the coordinates round) and by tri_hit's margin at the far end of the hit range (1e-5 x 350 x sqrt 3)
    const F3 c = 0.5f * (lo + hi), e = hi - lo;
    float r = 0.5f * sqrtf(dot(e, e));
    r = r * 1.0001f + 1.2e-2f + 4e-6f * (fabsf(c.x) + fabsf(c.y) + fabsf(c.z));
    S.sphere[n] = make_float4(c.x, c.y, c.z, r);
    if (S.R.nprims > 0) key = min_key(c.z - r);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s));
  if ((threadIdx.x & 63) == 0 && key != 0xffffffffu) atomicMin(S.zmin, key);
}

// the ray in one body's frame, and what the body's tests share
struct BodyRay {
  F3 o, d, inv;   // inv: 1 / d, 0 where d is 0
  float m, M;     // tri_hit's and box_near's margins
};
__device__ __forceinline__ BodyRay body_ray(const BodyFrame& B, F3 o, F3 d, float radius) {
  BodyRay r;
  r.o = to_body(B, o - f3(B.p[0], B.p[1], B.p[2]));
  r.d = to_body(B, d);
  r.inv = f3(r.d.x != 0.0f ? 1.0f / r.d.x : 0.0f, r.d.y != 0.0f ? 1.0f / r.d.y : 0.0f, r.d.z != 0.0f ? 1.0f / r.d.z : 0.0f);
  const float s = fabsf(r.o.x) + fabsf(r.o.y) + fabsf(r.o.z) + radius;
  r.m = TRI_MARGIN * s;
  r.M = BOX_MARGIN * s;
  return r;
}

// Slab test of the box (lo, hi) widened by r.M: true when the line is inside it somewhere in [tlo, thi]; tn: where it
// enters.  A direction component of exactly 0 tests the origin against the slab.
__device__ __forceinline__ bool box_near(const BodyRay& r, F3 lo, F3 hi, float tlo, float thi, float& tn) {
  float tf = INFINITY;
  tn = -INFINITY;
  bool miss = false;
#define T1_SLAB(c)                                                      \
  if (r.d.c != 0.0f) {                                                  \
    const float t1 = (lo.c - r.M - r.o.c) * r.inv.c, t2 = (hi.c + r.M - r.o.c) * r.inv.c; \
    tn = fmaxf(tn, fminf(t1, t2));                                      \
    tf = fminf(tf, fmaxf(t1, t2));                                      \
  } else if (r.o.c < lo.c - r.M || r.o.c > hi.c + r.M) {                \
    miss = true;                                                        \
  }
  T1_SLAB(x) T1_SLAB(y) T1_SLAB(z)
#undef T1_SLAB
  return !miss && tn <= tf && tn <= thi && tf >= tlo;
}

struct Node {
  F3 lo, hi;
  int a, b;
};
__device__ __forceinline__ Node load_node(const MeshDev& M, int i) {
  const float4 p = M.nodes[2 * (size_t)i], q = M.nodes[2 * (size_t)i + 1];
  return Node{f3(p.x, p.y, p.z), f3(p.w, q.x, q.y), __float_as_int(q.z), __float_as_int(q.w)};
}
struct Tri {
  F3 v0, e1, e2;
  int idx, body;
  uint32_t rgb;
};
__device__ __forceinline__ Tri load_tri(const MeshDev& M, int i) {
  const float4 p = M.tris[3 * (size_t)i], q = M.tris[3 * (size_t)i + 1], s = M.tris[3 * (size_t)i + 2];
  return Tri{f3(p.x, p.y, p.z), f3(p.w, q.x, q.y), f3(q.z, q.w, s.x), __float_as_int(s.y), __float_as_int(s.w),
             __float_as_uint(s.z)};
}

// Moeller-Trumbore, two-sided, the edges widened by EDGE_TOL (barycentric) so that a ray along an edge two triangles
// share cannot slip between them.  A hit counts at t in (tlo, thi] and only at a point inside the triangle's own box
// widened by r.m (the file's head).  A triangle of zero area has zero edges, so det == 0.
__device__ __forceinline__ bool tri_hit(const BodyRay& r, const Tri& T, float tlo, float thi, float& t) {
  const F3 pv = cross(r.d, T.e2);
  const float det = dot(T.e1, pv);
  if (det == 0.0f) return false;
  const float inv = 1.0f / det;
  const F3 tv = r.o - T.v0;
  const float u = dot(tv, pv) * inv;
  if (!(u >= -EDGE_TOL && u <= 1.0f + EDGE_TOL)) return false;
  const F3 qv = cross(tv, T.e1);
  const float v = dot(r.d, qv) * inv;
  if (!(v >= -EDGE_TOL && u + v <= 1.0f + EDGE_TOL)) return false;
  t = dot(T.e2, qv) * inv;
  if (!(t > tlo && t <= thi)) return false;
  const F3 p = r.o + t * r.d, a = T.v0, b = T.v0 + T.e1, c = T.v0 + T.e2;
  return p.x >= fminf(a.x, fminf(b.x, c.x)) - r.m && p.x <= fmaxf(a.x, fmaxf(b.x, c.x)) + r.m &&
         p.y >= fminf(a.y, fminf(b.y, c.y)) - r.m && p.y <= fmaxf(a.y, fmaxf(b.y, c.y)) + r.m &&
         p.z >= fminf(a.z, fminf(b.z, c.z)) - r.m && p.z <= fmaxf(a.z, fmaxf(b.z, c.z)) + r.m;
}

// the camera ray's nearest hit so far: (t, env, caller's index) is what is minimised; pos is the triangle's place in
// leaf order, -1 before the first hit
struct Best {
  float t;
  int env, idx, pos;
};
__device__ __forceinline__ void take(Best& B, float t, int env, const Tri& T, int pos) {
  // envs come in ascending order: at equal t a hit of the same env wins by the lower caller's index, a later env never
  if (B.pos < 0 || t < B.t || (t == B.t && env == B.env && T.idx < B.idx)) B = Best{t, env, T.idx, pos};
}

// One body against one ray.  ANY: the shadow ray -- true at the first triangle hit at t in (0, T_MAX].  Else the camera
// ray: B is updated, the walk prunes against B.t.  stk: the lane's stack (stride CHUNK).
template <bool ANY>
__device__ bool cast_body(const MeshDev& M, int b, const BodyRay& r, int env, Best& B, int32_t* stk, bool brute) {
  const float tlo = ANY ? 0.0f : T_MIN;
  float tn;
  Node N = load_node(M, M.root[b]);
  if (!box_near(r, N.lo, N.hi, tlo, ANY ? T_MAX : B.t, tn)) return false;
  if (brute) {
    for (int i = M.first[b]; i < M.first[b] + M.count[b]; ++i) {
      const Tri T = load_tri(M, i);
      float t;
      if (tri_hit(r, T, tlo, T_MAX, t)) {
        if (ANY) return true;
        take(B, t, env, T, i);
      }
    }
    return false;
  }
  int sp = 0;
  for (;;) {
    if (N.b > 0) {   // a leaf
      for (int i = N.a; i < N.a + N.b; ++i) {
        const Tri T = load_tri(M, i);
        float t;
        if (tri_hit(r, T, tlo, T_MAX, t)) {
          if (ANY) return true;
          take(B, t, env, T, i);
        }
      }
    } else {
      const Node L = load_node(M, N.a), R = load_node(M, N.a + 1);
      float tl, tr;
      const float thi = ANY ? T_MAX : B.t;
      const bool hl = box_near(r, L.lo, L.hi, tlo, thi, tl), hr = box_near(r, R.lo, R.hi, tlo, thi, tr);
      if (hl && hr) {
        const bool left_first = tl <= tr;
        if (sp < STACK) stk[CHUNK * sp++] = N.a + (left_first ? 1 : 0);   // sp < STACK always: the builder's depth bound
        N = left_first ? L : R;
        continue;
      }
      if (hl || hr) {
        N = hl ? L : R;
        continue;
      }
    }
    if (sp == 0) return false;
    N = load_node(M, stk[CHUNK * --sp]);
  }
}

// Poses the next batch of envs into LDS and returns its size, 0 when the scene is exhausted.  With OTHERS the envs come
// from the tile-level scan; without, the camera's env is the whole scene.  Every decision in it is uniform.
__device__ int next_batch(Batch& S, const MeshArgs& A, const Frustum& Fr, float z_floor, int cam, int tid, Cursor& c) {
  __syncthreads();   // every lane is done with the previous batch
  const SceneArgs& Sc = A.S;
  int ne;
  if (Sc.flags & T1RENDER_SCENE_OTHERS) {
    if (!scan_on(S.scan, Sc, Fr, z_floor, cam, tid, c)) return 0;
    ne = min(BATCH_ENVS, c.m - c.sb);
  } else {
    if (c.base > 0) return 0;
    c.base = 1;
    ne = 1;
    if (tid == 0) S.scan.surv[0] = Sc.R.cams[cam].env;
    __syncthreads();
  }
  const int slot = tid / NB, b = tid % NB;
  if (slot < ne) {
    const int env = S.scan.surv[c.sb + slot];
    pose_body(S.body[slot * NB + b], Sc.R.rigid_state + (size_t)env * 169 + 13 * b);
    if (b == 0) S.env[slot] = env;
  }
  c.sb += ne;
  __syncthreads();
  return ne;
}

__global__ __launch_bounds__(CHUNK) void k_mesh(const MeshArgs A) {
  __shared__ Batch S;
  const SceneArgs& Sc = A.S;
  const RenderArgs& R = Sc.R;
  const MeshDev& M = A.M;
  const int tid = threadIdx.y * TILE + threadIdx.x, cam = blockIdx.z;
  if (tid == 0) camera_frame(S.cam, R, cam);
  __syncthreads();
  const int j = blockIdx.x * TILE + threadIdx.x, i = blockIdx.y * TILE + threadIdx.y;
  const bool inside = j < R.width && i < R.height;   // edge tiles: no store outside the image
  const bool cull = (Sc.flags & T1RENDER_SCENE_OTHERS) && !(Sc.flags & T1RENDER_SCENE_BRUTE);
  const bool brute = Sc.flags & T1RENDER_MESH_BRUTE;
  const Frustum Fr = make_frustum(S.cam, 2.0f * (float)(blockIdx.x * TILE) / (float)R.width - 1.0f,
                                  2.0f * (float)(blockIdx.x * TILE + TILE) / (float)R.width - 1.0f,
                                  1.0f - 2.0f * (float)(blockIdx.y * TILE + TILE) / (float)R.height,
                                  1.0f - 2.0f * (float)(blockIdx.y * TILE) / (float)R.height);
  const float z_floor = cull ? scene_floor(Sc) : 0.0f;
  const F3 o = f3(S.cam.eye[0], S.cam.eye[1], S.cam.eye[2]), d = pixel_ray(S.cam, R, i, j);
  int32_t* stk = S.stack + tid;
  Best B = {T_MAX, -1, -1, -1};
  Cursor cur = {0, 0, 0};
  if (R.nprims > 0) {
    for (int ne = next_batch(S, A, Fr, z_floor, cam, tid, cur); ne > 0; ne = next_batch(S, A, Fr, z_floor, cam, tid, cur)) {
      if (!inside) continue;
      for (int s = 0; s < ne; ++s) {
        const int env = S.env[s];
        for (int b = 0; b < NB; ++b) {
          if (M.root[b] < 0) continue;
          const BodyRay r = body_ray(S.body[s * NB + b], o, d, M.radius[b]);
          cast_body<false>(M, b, r, env, B, stk, brute);
        }
      }
    }
  }
  Surface h = {f3(0, 0, 1), f3(0, 0, 0), f3(0, 0, 0), f3(0, 0, 0), 0.0f, -1, false, false};
  float best = B.t;
  int henv = B.env, htri = -1;
  if (inside)
    h = surface(R, o, d, best, B.pos, henv, [&](Surface& h, F3) {
      // the batch that held the body's frame is gone: pose it again
      const Tri T = load_tri(M, B.pos);
      BodyFrame F;
      pose_body(F, R.rigid_state + (size_t)B.env * 169 + 13 * T.body);
      F3 n = normalize(to_world(F, cross(T.e1, T.e2)));
      if (dot(n, d) > 0.0f) n = -1.0f * n;   // flat shading, the side the ray came from
      h.n = n;
      h.base = f3((float)(T.rgb & 255u) * (1.0f / 255.0f), (float)((T.rgb >> 8) & 255u) * (1.0f / 255.0f),
                  (float)((T.rgb >> 16) & 255u) * (1.0f / 255.0f));
      h.id = 1 + T.body;
      htri = T.idx;
    });
  float lit = 1.0f;
  if (R.nprims > 0 && __syncthreads_or(h.need)) {   // the shadow rays against the same scene
    const F3 L = f3(R.style.light[0], R.style.light[1], R.style.light[2]);
    cur = Cursor{0, 0, 0};
    for (int ne = next_batch(S, A, Fr, z_floor, cam, tid, cur); ne > 0; ne = next_batch(S, A, Fr, z_floor, cam, tid, cur)) {
      if (!h.need || lit == 0.0f) continue;
      for (int s = 0; s < ne && lit != 0.0f; ++s) {
        for (int b = 0; b < NB && lit != 0.0f; ++b) {
          if (M.root[b] < 0) continue;
          const BodyRay r = body_ray(S.body[s * NB + b], h.so, L, M.radius[b]);
          if (cast_body<true>(M, b, r, 0, B, stk, brute)) lit = 0.0f;
        }
      }
    }
  }
  if (inside) {
    store_pixel(Sc, h, lit, best, henv, cam, i, j);
    if (A.tris_out) A.tris_out[((size_t)cam * R.height + i) * R.width + j] = henv >= 0 ? htri : -1;
  }
}

std::mutex g_live_mutex;
std::set<const t1render_mesh*> g_live;   // handles created and not yet destroyed

bool is_live(const t1render_mesh* m) {
  std::lock_guard<std::mutex> lock(g_live_mutex);
  return g_live.count(m) != 0;
}

}  // namespace

extern "C" int t1render_mesh_create(const float* tri, const int32_t* body, const uint32_t* rgb, int32_t ntri,
                                    t1render_mesh** out) {
  if (!out) return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: null out");
  *out = nullptr;
  if (ntri < 0 || ntri > t1bvh::MAX_TRI) return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: ntri outside [0, 2^20]");
  if (!tri || !body || !rgb) return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: null argument");
  t1bvh::Mesh H;
  switch (t1bvh::build(tri, body, rgb, ntri, &H)) {
    case t1bvh::OK: break;
    case t1bvh::E_BODY: return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: a triangle's body is outside [0, 13)");
    case t1bvh::E_FINITE: return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: a vertex is not finite");
    default: return t1_fail(T1ENV_E_ARG, "t1render_mesh_create: the mesh is refused");
  }
  t1render_mesh* m = new t1render_mesh();
  m->ntri = ntri;
  m->nnodes = (int32_t)H.nodes.size();
  m->max_depth = H.max_depth;
  for (int b = 0; b < NB; ++b) {
    m->root[b] = H.root[b];
    m->first[b] = H.first[b];
    m->count[b] = H.count[b];
    m->radius[b] = H.radius[b];
  }
  hipError_t err = hipSuccess;
  if (ntri > 0) {
    const size_t nb = H.nodes.size() * sizeof(t1bvh::Node), tb = H.tris.size() * sizeof(t1bvh::Tri);
    err = hipMalloc((void**)&m->nodes, nb);
    if (err == hipSuccess) err = hipMalloc((void**)&m->tris, tb);
    if (err == hipSuccess) err = hipMemcpy(m->nodes, H.nodes.data(), nb, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(m->tris, H.tris.data(), tb, hipMemcpyHostToDevice);
  }
  if (err != hipSuccess) {
    if (m->nodes) (void)hipFree(m->nodes);
    if (m->tris) (void)hipFree(m->tris);
    delete m;
    return t1_fail((int)err, hipGetErrorString(err));
  }
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.insert(m);
  }
  *out = m;
  return 0;
}

extern "C" int t1render_mesh_destroy(t1render_mesh* m) {
  if (!m) return 0;
  {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    if (!g_live.erase(m)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_destroy: not a live mesh handle");
  }
  if (m->nodes) (void)hipFree(m->nodes);
  if (m->tris) (void)hipFree(m->tris);
  delete m;
  return 0;
}

extern "C" int t1render_mesh_info(const t1render_mesh* m, int32_t* ntri, int32_t* nnodes, int32_t* max_depth,
                                  float* radius) {
  if (!m || !is_live(m)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_info: not a live mesh handle");
  if (ntri) *ntri = m->ntri;
  if (nnodes) *nnodes = m->nnodes;
  if (max_depth) *max_depth = m->max_depth;
  if (radius)
    for (int b = 0; b < NB; ++b) radius[b] = m->radius[b];
  return 0;
}

extern "C" long long t1render_mesh_workspace_bytes(int32_t num_envs, int32_t ncams) {
  if (num_envs < 0 || ncams < 1 || ncams > T1RENDER_MAXCAM) return -1;
  return scene_workspace_bytes(num_envs, ncams, nullptr);
}

extern "C" int t1render_mesh_scene(t1env* env, const t1render_camera* cams, int32_t ncams, const t1render_mesh* mesh,
                                   const t1render_style* style, int32_t flags, int32_t width, int32_t height,
                                   uint32_t* rgba, float* depth, int32_t* ids, int32_t* envs, int32_t* tris,
                                   void* workspace, long long workspace_bytes_, void* stream) {
  if (!env || !cams || !mesh || !style || !rgba) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: null argument");
  if (!is_live(mesh)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: not a live mesh handle");
  if (ncams < 1 || ncams > T1RENDER_MAXCAM) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: ncams outside [1, 16]");
  if (width < 1 || height < 1) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: width and height must be >= 1");
  if (flags & ~FLAGS_ALL) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: unknown flag");
  RenderView v;
  t1_render_view(env, &v);
  MeshArgs A = {};
  SceneArgs& S = A.S;
  RenderArgs& R = S.R;
  for (int c = 0; c < ncams; ++c) {
    const t1render_camera& C = cams[c];
    if (C.env < 0 || C.env >= v.num_envs) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: a camera's env is out of range");
    // follow mode adds the same base position to eye and target: the view direction is that of the offsets
    const double f[3] = {(double)C.target[0] - C.eye[0], (double)C.target[1] - C.eye[1], (double)C.target[2] - C.eye[2]};
    const double u[3] = {C.up[0], C.up[1], C.up[2]};
    const double x[3] = {f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0]};
    const double ff = f[0] * f[0] + f[1] * f[1] + f[2] * f[2], uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double xx = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(xx > 1e-12 * ff * uu)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: a camera's up is parallel to its view");
    if (!(C.vfov > 0.0f && C.vfov < 3.14159f)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: vfov outside (0, pi)");
    R.cams[c] = C;
  }
  if (v.terrain.type != 0 && !v.terrain.h) return t1_fail(T1ENV_E_STATE, "t1render_mesh_scene: no terrain set");
  R.style = *style;
  const double ll = sqrt((double)style->light[0] * style->light[0] + (double)style->light[1] * style->light[1] +
                         (double)style->light[2] * style->light[2]);
  if (!(ll > 0.0)) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: zero light direction");
  for (int k = 0; k < 3; ++k) R.style.light[k] = (float)(style->light[k] / ll);
  const bool cull = (flags & T1RENDER_SCENE_OTHERS) && !(flags & T1RENDER_SCENE_BRUTE);
  long long words = 0;
  const long long need = scene_workspace_bytes(v.num_envs, ncams, &words);
  if (cull && !workspace) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: OTHERS needs a workspace");
  if (workspace) {
    if ((uintptr_t)workspace % 16) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: the workspace is not 16-byte aligned");
    if (workspace_bytes_ < need) return t1_fail(T1ENV_E_ARG, "t1render_mesh_scene: the workspace is smaller than t1render_mesh_workspace_bytes");
  }
  R.rigid_state = v.rigid_state;
  R.h = v.terrain.h;
  R.rows = v.terrain.rows;
  R.cols = v.terrain.cols;
  R.hf = v.terrain.type != 0;
  R.inv_hscale = v.terrain.inv_hscale;
  R.hscale = v.terrain.hscale;
  R.vscale = v.terrain.vscale;
  R.border = v.terrain.border;
  R.z_top = v.z_top + 1e-3f * (1.0f + fabsf(v.z_top));
  R.width = width;
  R.height = height;
  R.nprims = mesh->ntri > 0 ? 1 : 0;
  R.rgba = rgba;
  R.depth = depth;
  R.ids = ids;
  S.envs = envs;
  S.flags = flags;
  S.num_envs = v.num_envs;
  S.ncams = ncams;
  S.words = (int32_t)words;
  S.z_bot = v.z_bot - 1e-3f * (1.0f + fabsf(v.z_bot));
  A.M.nodes = mesh->nodes;
  A.M.tris = mesh->tris;
  for (int b = 0; b < NB; ++b) {
    A.M.root[b] = mesh->root[b];
    A.M.first[b] = mesh->first[b];
    A.M.count[b] = mesh->count[b];
    A.M.radius[b] = mesh->radius[b];
  }
  A.tris_out = tris;
  const hipStream_t st = (hipStream_t)stream;
  if (cull) {
    char* ws = (char*)workspace;
    S.sphere = (float4*)ws;
    S.bits = (uint32_t*)(ws + 16 * (size_t)v.num_envs);
    S.zmin = S.bits + (size_t)ncams * words;
    hipError_t err = hipMemsetAsync(S.zmin, 0xff, sizeof(uint32_t), st);
    if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
    const dim3 pre((v.num_envs + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(k_mesh_bounds, pre, dim3(CHUNK), 0, st, A);
    hipLaunchKernelGGL(k_scene_bits, pre, dim3(CHUNK), 0, st, S);
    err = hipGetLastError();
    if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  }
  const dim3 grid((width + TILE - 1) / TILE, (height + TILE - 1) / TILE, ncams);
  hipLaunchKernelGGL(k_mesh, grid, dim3(TILE, TILE), 0, st, A);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return t1_fail((int)err, hipGetErrorString(err));
  return 0;
}
