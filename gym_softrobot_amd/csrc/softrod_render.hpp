// softrod_render.hpp — softrod_render_kernel: batched RGB and depth frames of the resident rods (softrod_render).
//
// A cold kernel beside the read-outs: it reads the resident state and writes the two frame buffers only.  When a policy
// consumes pixels it becomes the hot path of the loop, so it is a software rasteriser written for gfx950 and not a torch
// composite.  The image model — orthographic camera, pixel centres, the primitive list and its order, coverage, depth,
// tie rule, colour, what a non-finite primitive does — is the contract in include/softrod.h (softrod_render); this file
// says how the kernel keeps it.
//
// THE IMPOSTOR.  A capsule is drawn as the sphere swept along the PROJECTED segment: the nearest point q of the segment
// to the pixel is found in the image plane, the surface is h = sqrt(r^2 - |p - q|^2) in front of q's depth.  That is exact
// for the silhouette, and exact for the depth where the element is perpendicular to the view; an element tilted towards
// the viewer is drawn slightly too near at its far flank.  A sphere is the capsule with A = B.
//
// ONE WORKGROUP of kRenderThreads = 256 lanes per (pixel tile, env); a tile is kRenderTileW x kRenderTileH = 32 x 32
// pixels, blockIdx.x = env * tiles + tile.
//   1. Project, cull, compact — in chunks of 256 primitives, in primitive order.  Lane t of the workgroup takes primitive
//      chunk + t: it reads the two end points from the float64 rows (readout_rod's addressing: slot arm * arm_stride + node
//      of the env's row), subtracts the camera centre (plus the env's anchor with `follow`) and projects IN FLOAT64 — a
//      crawling octopus may be far from the origin — and only then rounds to float32.  It keeps the primitive iff every
//      staged number is finite in float32, r > 0 and the primitive's bounding rectangle, grown by r and a slack far above
//      float32 rounding, meets the tile's rectangle of pixel centres.  Every test is written as a comparison that is FALSE
//      for a NaN, so a primitive with a non-finite coordinate or radius is dropped here and covers no pixel; there is no
//      float-to-int conversion anywhere (tiles are compared as float rectangles, not binned).
//      The survivors of a chunk are compacted with a wave ballot and a prefix over the four waves' counts (LDS), so the
//      staged list is in primitive order whatever the scheduling: the tie rule "lowest index wins" is then the strict `>` of
//      the depth test, with no extra compare and no atomics.
//      A staged primitive is twelve 32-bit words (three 16-byte LDS slots):
//          Au Av Du Dv | wA Dw 1/|D|^2 r | r^2 1/r colour body        D = B - A; 1/|D|^2 = 0 for a sphere
//      The LDS array is sized by the host from the handle's own primitive count (dynamic LDS, 32 + 48 n_prims bytes; at
//      most kRenderMaxPrims = 8 x 126 + 2, softrod_render refuses a handle beyond it) and a slot is written only below
//      that count.
//   2. Shade — each lane owns kRenderPx = 4 horizontally adjacent pixels of one row (8 lanes per 32-pixel row, a wave
//      covers 8 rows, each row's 96 RGB bytes contiguous) and walks the compacted list once; every lane reads the same
//      primitive (an LDS broadcast).  A wave skips, as a whole, a primitive whose v range grown by r misses its 8 rows
//      (the same conservative rectangle test as the tile's cull: skipping changes no pixel).  The winner's p - q, h,
//      1/r and colour stay in registers; the colour is shaded after the loop.
//   3. Store — with W % 4 == 0 (and 4- / 16-byte aligned buffers) a lane's 12 RGB bytes go out as three aligned 32-bit
//      stores and its four depths as one float4; otherwise byte / float stores per pixel.  The last tile column and row
//      are masked, not padded.
//
// PRECISION.  Everything per pixel is float32.  The projected coordinates are of the order of the half width, so they
// carry ~1e-7 of it; the tests skip the pixels whose float64 answer hinges on less than 1e-4 (tests/render_ref.py).
#pragma once

#include <float.h>

namespace softrod {

constexpr int kRenderThreads = 256;
constexpr int kRenderTileW = 32, kRenderTileH = 32;
constexpr int kRenderPx = 4;                       // pixels per lane
constexpr int kRenderMaxPrims = 8 * 126 + 2;       // 8 arms of 126 elements, head, target
constexpr int kRenderBodies = 10;                  // palette entries: arm index mod 8, head, target
constexpr int kRenderPrimWords = 12;
constexpr int kRenderLdsHeader = 8;                // words in front of the staged list: the four waves' counts
static_assert(kRenderTileW * kRenderTileH == kRenderThreads * kRenderPx, "a lane owns kRenderPx pixels of the tile");

__constant__ uint32_t kRenderPalette[kRenderBodies] = SOFTROD_RENDER_PALETTE;   // 0xRRGGBB

inline size_t render_lds_bytes(int n_prims) {
    return (size_t)(kRenderLdsHeader + kRenderPrimWords * n_prims) * sizeof(float);
}

// The camera as the kernel takes it: the float64 part for the projection, the rest already float32.
struct RenderCamera {
    double c[3], a[3], b[3], n[3];     // centre, right, up, towards the viewer (a x b)
    float half_width, target_radius, ambient;
    float light[3];
    int width, height, follow;
};

// An env's target point, where its kind has one: what softrod_render draws and softrod_rod_clearance measures to (the
// host fills it in env_target, softrod_capi.hip).  kind: 0 none, 1 `constant` (z = 0), 2 rows of `rows` ([dims][n_envs],
// z = 0 with dims == 2).
struct EnvTarget {
    const double* rows;
    double constant[2];
    int kind, dims;
};
__device__ __forceinline__ void env_target_point(const EnvTarget& T, size_t N, int env, double X[3]) {
    if (T.kind == 1) {
        X[0] = T.constant[0]; X[1] = T.constant[1]; X[2] = 0.0;
    } else {
        X[0] = T.rows[env]; X[1] = T.rows[N + env];
        X[2] = T.dims == 3 ? T.rows[2 * N + env] : 0.0;
    }
}

// What of the handle the kernel reads.
struct RenderScene {
    const double* pos;        // [3][n_envs][lane_stride]
    const double* head;       // [20][n_envs], rows 0-2 the rigid body's position; nullptr: no head
    const double* radius;     // [n_elem] rest radius of every element
    EnvTarget target;
    float head_radius;
    int n_envs, n_elem, rods, lane_stride, arm_stride;
    int n_prims;
};

__device__ __forceinline__ bool render_finite(float x) { return fabsf(x) <= FLT_MAX; }    // false for NaN and +-inf

__global__ void __launch_bounds__(kRenderThreads)
softrod_render_kernel(const RenderScene sc, const RenderCamera cam, uint8_t* __restrict__ rgb, float* __restrict__ depth,
                      const int tiles_x, const int tiles_y, const int wide) {
    extern __shared__ float4 render_lds[];
    int* counts = reinterpret_cast<int*>(render_lds);                         // [4]
    float4* prims = render_lds + kRenderLdsHeader / 4;                        // [n_prims][3]
    const int tid = threadIdx.x, lane = tid & (kLanes - 1), wave = tid / kLanes;
    const int tiles = tiles_x * tiles_y;
    const int env = blockIdx.x / tiles, tile = blockIdx.x - env * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int W = cam.width, H = cam.height;
    const size_t N = (size_t)sc.n_envs, LS = (size_t)sc.lane_stride;

    // pixel centres, float32 (include/softrod.h "Pixels")
    const float su = 2.0f / (float)W, sv = 2.0f / (float)H;
    const float hw = cam.half_width, hh = cam.half_width * (float)H / (float)W;
    const int x0 = tx * kRenderTileW, y0 = ty * kRenderTileH;
    const int x1 = min(x0 + kRenderTileW, W) - 1, y1 = min(y0 + kRenderTileH, H) - 1;
    const float slack = 1e-5f * hw;
    const float umin = (((float)x0 + 0.5f) * su - 1.0f) * hw - slack, umax = (((float)x1 + 0.5f) * su - 1.0f) * hw + slack;
    const float vmax = (1.0f - ((float)y0 + 0.5f) * sv) * hh + slack, vmin = (1.0f - ((float)y1 + 0.5f) * sv) * hh - slack;

    // the centre the env's points are taken from, float64
    double c[3] = {cam.c[0], cam.c[1], cam.c[2]};
    if (cam.follow) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            c[k] += sc.head ? sc.head[(size_t)k * N + env] : sc.pos[((size_t)k * N + env) * LS];
    }
    auto project = [&](const double X[3], float& u, float& v, float& w) {
        const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
        u = (float)(d0 * cam.a[0] + d1 * cam.a[1] + d2 * cam.a[2]);
        v = (float)(d0 * cam.b[0] + d1 * cam.b[1] + d2 * cam.b[2]);
        w = (float)(d0 * cam.n[0] + d1 * cam.n[1] + d2 * cam.n[2]);
    };

    // 1. project, cull, compact: in primitive order
    const int n_caps = sc.rods * sc.n_elem;
    int total = 0;                                                            // uniform over the workgroup
    for (int chunk = 0; chunk < sc.n_prims; chunk += kRenderThreads) {
        const int p = chunk + tid;
        bool keep = false;
        float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0, f2 = f0;
        if (p < sc.n_prims) {
            double A[3], B[3];
            float r;
            int body;
            if (p < n_caps) {
                const int arm = p / sc.n_elem, k = p - arm * sc.n_elem;
                const size_t i = (size_t)env * LS + (size_t)arm * (size_t)sc.arm_stride + (size_t)k;
#pragma unroll
                for (int q = 0; q < 3; ++q) { A[q] = sc.pos[(size_t)q * N * LS + i]; B[q] = sc.pos[(size_t)q * N * LS + i + 1]; }
                r = (float)sc.radius[k];
                body = arm & 7;
            } else if (p == n_caps && sc.head) {
#pragma unroll
                for (int q = 0; q < 3; ++q) A[q] = B[q] = sc.head[(size_t)q * N + env];
                r = sc.head_radius;
                body = 8;
            } else {
                env_target_point(sc.target, N, env, A);
#pragma unroll
                for (int q = 0; q < 3; ++q) B[q] = A[q];
                r = cam.target_radius;
                body = 9;
            }
            float au, av, aw, bu, bv, bw;
            project(A, au, av, aw);
            project(B, bu, bv, bw);
            const float du = bu - au, dv = bv - av, l2 = du * du + dv * dv;
            const bool finite = render_finite(au) && render_finite(av) && render_finite(aw) && render_finite(bu) &&
                                render_finite(bv) && render_finite(bw) && render_finite(r);
            keep = finite && r > 0.0f && fminf(au, bu) - r <= umax && fmaxf(au, bu) + r >= umin &&
                   fminf(av, bv) - r <= vmax && fmaxf(av, bv) + r >= vmin;
            f0 = make_float4(au, av, du, dv);
            f1 = make_float4(aw, bw - aw, l2 > 0.0f ? 1.0f / l2 : 0.0f, r);
            f2 = make_float4(r * r, 1.0f / r, __uint_as_float(kRenderPalette[body]), __int_as_float(body));
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) counts[wave] = __popcll(m);
        __syncthreads();
        int slot = total + __popcll(m & ((1ull << lane) - 1ull));
        int chunk_total = 0;
#pragma unroll
        for (int w = 0; w < kRenderThreads / kLanes; ++w) {
            const int cw = counts[w];
            if (w < wave) slot += cw;
            chunk_total += cw;
        }
        if (keep && slot < sc.n_prims) { prims[3 * slot] = f0; prims[3 * slot + 1] = f1; prims[3 * slot + 2] = f2; }
        total += chunk_total;
        __syncthreads();
    }
    total = min(total, sc.n_prims);

    // 2. shade: this lane's four pixels over the compacted list
    const int row = y0 + tid / (kRenderTileW / kRenderPx);
    const int col0 = x0 + (tid % (kRenderTileW / kRenderPx)) * kRenderPx;
    const float pv = (1.0f - ((float)row + 0.5f) * sv) * hh;
    float pu[kRenderPx], zb[kRenderPx], qu[kRenderPx], qv[kRenderPx], hb[kRenderPx];
    int win[kRenderPx];
#pragma unroll
    for (int i = 0; i < kRenderPx; ++i) {
        pu[i] = (((float)(col0 + i) + 0.5f) * su - 1.0f) * hw;
        zb[i] = -INFINITY; qu[i] = qv[i] = hb[i] = 0.0f; win[i] = -1;
    }
    // this wave's strip of the tile (8 rows): a primitive whose v range, grown by r, misses it is skipped by the whole wave
    const int strip0 = y0 + wave * (kLanes / (kRenderTileW / kRenderPx));
    const int strip1 = min(strip0 + kLanes / (kRenderTileW / kRenderPx), H) - 1;
    const float svmax = (1.0f - ((float)strip0 + 0.5f) * sv) * hh + slack, svmin = (1.0f - ((float)strip1 + 0.5f) * sv) * hh - slack;
    if (strip0 >= H) total = 0;
    for (int k = 0; k < total; ++k) {
        const float4 f0 = prims[3 * k], f1 = prims[3 * k + 1];
        const float bv = f0.y + f0.w;
        if (fminf(f0.y, bv) - f1.w > svmax || fmaxf(f0.y, bv) + f1.w < svmin) continue;      // (wave-uniform)
        const float r2 = prims[3 * k + 2].x;
        const float ev = pv - f0.y;
#pragma unroll
        for (int i = 0; i < kRenderPx; ++i) {
            const float eu = pu[i] - f0.x;
            const float t = fminf(fmaxf((eu * f0.z + ev * f0.w) * f1.z, 0.0f), 1.0f);
            const float gu = eu - t * f0.z, gv = ev - t * f0.w;                // p - q
            const float d2 = gu * gu + gv * gv;
            const float h = sqrtf(fmaxf(r2 - d2, 0.0f));
            const float z = f1.x + t * f1.y + h;
            if (d2 < r2 && z > zb[i]) { zb[i] = z; qu[i] = gu; qv[i] = gv; hb[i] = h; win[i] = k; }   // false for a NaN
        }
    }

    // 3. colour and store
    if (row >= H || col0 >= W) return;
    uint8_t px[kRenderPx][3];
#pragma unroll
    for (int i = 0; i < kRenderPx; ++i) {
        uint32_t colour = SOFTROD_RENDER_BACKGROUND;
        float shade = 1.0f;
        if (win[i] >= 0) {
            const float4 f2 = prims[3 * win[i] + 2];
            const float lam = fmaxf(0.0f, (qu[i] * cam.light[0] + qv[i] * cam.light[1] + hb[i] * cam.light[2]) * f2.y);
            shade = cam.ambient + (1.0f - cam.ambient) * lam;
            colour = __float_as_uint(f2.z);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float x = (float)((colour >> (16 - 8 * ch)) & 255u) * (1.0f / 255.0f) * shade;
            px[i][ch] = (uint8_t)fminf(fmaxf(floorf(255.0f * x + 0.5f), 0.0f), 255.0f);
        }
    }
    const size_t pix = ((size_t)env * (size_t)H + (size_t)row) * (size_t)W + (size_t)col0;
    if (wide) {     // W % 4 == 0: the four pixels are all inside, 12 bytes at a multiple of 12, 16 bytes of depth at a multiple of 16
        uint32_t* out = reinterpret_cast<uint32_t*>(rgb + pix * 3);
        out[0] = (uint32_t)px[0][0] | (uint32_t)px[0][1] << 8 | (uint32_t)px[0][2] << 16 | (uint32_t)px[1][0] << 24;
        out[1] = (uint32_t)px[1][1] | (uint32_t)px[1][2] << 8 | (uint32_t)px[2][0] << 16 | (uint32_t)px[2][1] << 24;
        out[2] = (uint32_t)px[2][2] | (uint32_t)px[3][0] << 8 | (uint32_t)px[3][1] << 16 | (uint32_t)px[3][2] << 24;
        if (depth) *reinterpret_cast<float4*>(depth + pix) = make_float4(zb[0], zb[1], zb[2], zb[3]);
    } else {
#pragma unroll
        for (int i = 0; i < kRenderPx; ++i) {
            if (col0 + i < W) {
                rgb[(pix + i) * 3] = px[i][0]; rgb[(pix + i) * 3 + 1] = px[i][1]; rgb[(pix + i) * 3 + 2] = px[i][2];
                if (depth) depth[pix + i] = zb[i];
            }
        }
    }
}

}  // namespace softrod
