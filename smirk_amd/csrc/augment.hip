// Parameter augmentation of the cycle path for MI355X (gfx950): the block smirk_trainer.py:192-248 runs at the start of every `step2` — about 150 eager
// launches on [Ke*B, 50] tensors plus one pageable host-to-device copy per template row — as two launches on the caller's stream, with no host
// synchronisation, no copy and no allocation.  The work is a few hundred KB: latency-bound, so the shape of the kernels is "few launches, no round trips".
//   augment_plan_kernel    one thread per output row: its key of the group permutation is ranked against all N keys, staged AUG_TILE at a time in LDS
//                          (every workgroup regenerates the keys from the counters: 10 Philox rounds are cheaper than a launch that would publish them);
//                          rank -> group (cut at N/4, 2N/4, 3N/4: smirk_trainer.py:200-202) and position in the group; template class and row (:220-222,
//                          base_trainer.py:69-74: class first, then a row of it); row_at[rank] = row and key2_at[rank] = the row's second key (workspace)
//   augment_apply_kernel   one 64-lane wave per output row: a row of group 1 ranks its second key among the rows of its group (read back through row_at /
//                          key2_at: the permutation inside the group, smirk_trainer.py:215) and takes the row at that position as its source; then the lanes
//                          loop over the columns: expression by group (:208-223,238-239), jaw (:226-228,241), eyelids (:231-233,242), copies of the rest.
// Draws: augment_rng.h (Philox streams 4 and 5, the counter layout and how many counters a call consumes).  Every discrete choice is a function of the
// integer draw, so tests/augment_law.py restates plan and outputs on the host from the same integers.
#include "common.h"
#include "augment_rng.h"

#define AUG_TILE 4096                                  // keys staged per pass (16 KB of LDS)
#define AUG_BLOCK 256

__global__ __launch_bounds__(AUG_BLOCK) void augment_plan_kernel(int N, int n_classes, const int32_t* __restrict__ class_off, uint64_t seed, uint64_t offset,
                                                                 int32_t* __restrict__ plan, int32_t* __restrict__ row_at, uint32_t* __restrict__ key2_at) {
    __shared__ uint32_t keys[AUG_TILE];
    const int r = blockIdx.x * AUG_BLOCK + threadIdx.x;
    const bool live = r < N;
    const AugDraw d = aug_philox(offset + 4ull * (uint64_t)(live ? r : 0), AUG_STREAM_ROW, seed);
    const uint32_t kr = d.x0;
    int rank = 0;
    for (int t0 = 0; t0 < N; t0 += AUG_TILE) {
        const int n = min(AUG_TILE, N - t0);
        __syncthreads();                               // the previous tile has been read by every wave
        for (int j = threadIdx.x; j < n; j += AUG_BLOCK) keys[j] = aug_philox(offset + 4ull * (uint64_t)(t0 + j), AUG_STREAM_ROW, seed).x0;
        __syncthreads();
        if (live) {
#pragma unroll 8
            for (int j = 0; j < n; ++j) {              // every lane reads the same word: an LDS broadcast
                const uint32_t kj = keys[j];
                rank += (int)((kj < kr) | ((kj == kr) & (t0 + j < r)));
            }
        }
    }
    if (!live) return;
    const int b1 = N / 4, b2 = 2 * N / 4, b3 = 3 * N / 4;
    const int g = (rank >= b1) + (rank >= b2) + (rank >= b3);
    const int start = g == 0 ? 0 : g == 1 ? b1 : g == 2 ? b2 : b3;
    int trow = -1;
    if (g == 2) {
        const int c = (int)(((uint64_t)d.x2 * (uint64_t)n_classes) >> 32);
        const int lo = class_off[c], hi = class_off[c + 1];
        trow = lo + (int)(((uint64_t)d.x3 * (uint64_t)(hi - lo)) >> 32);
    }
    plan[r * 4 + 0] = g;
    plan[r * 4 + 1] = rank - start;
    plan[r * 4 + 2] = -1;                              // group 1: the apply kernel fills in the source row
    plan[r * 4 + 3] = trow;
    row_at[rank] = r;
    key2_at[rank] = d.x1;
}

struct AugArgs {
    const float *expr, *jaw, *eyelid, *shape, *pose, *cam, *templates;
    float *o_expr, *o_jaw, *o_eyelid, *o_shape, *o_pose, *o_cam;
    int32_t* plan;
    const int32_t* row_at;
    const uint32_t* key2_at;
    uint64_t seed, offset;
    int B, N, E, S, num_expression, use_eyelids;
};

__global__ __launch_bounds__(AUG_BLOCK) void augment_apply_kernel(AugArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (AUG_BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= a.N) return;                              // wave-uniform
    const int b = r % a.B;
    const int g = a.plan[r * 4 + 0], trow = a.plan[r * 4 + 3];
    const uint64_t row_ctr = a.offset + 4ull * (uint64_t)r;

    int src = b;
    if (g == 1) {                                      // rank of this row's second key inside group 1 -> the row at that position is the source
        const int s1 = a.N / 4, e1 = 2 * a.N / 4;
        const uint32_t k2 = a.key2_at[s1 + a.plan[r * 4 + 1]];
        int cnt = 0;
        for (int p = s1 + lane; p < e1; p += 64) {
            const uint32_t kj = a.key2_at[p];
            cnt += (int)((kj < k2) | ((kj == k2) & (a.row_at[p] < r)));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        const int srow = a.row_at[s1 + cnt];
        if (lane == 0) a.plan[r * 4 + 2] = srow;
        src = srow % a.B;
    }

    const AugDraw ds = aug_philox(row_ctr + 1, AUG_STREAM_ROW, a.seed);
    const float u = aug_u01(ds.x0), noise = 0.2f * aug_u01(ds.x1);
    const float gain = g == 0 ? 1.0f + 2.0f * u : 0.25f + 1.25f * u;
    const float* e0 = a.expr + (size_t)b * a.E;
    const float* es = a.expr + (size_t)src * a.E;
    const float* tp = a.templates + (size_t)(trow < 0 ? 0 : trow) * a.num_expression;
    for (int c = lane; c < a.E; c += 64) {
        const AugDraw de = aug_philox(a.offset + (uint64_t)r * (uint64_t)a.E + (uint64_t)c, AUG_STREAM_ELEM, a.seed);
        float za, zb;
        aug_normal2(de.x0, de.x1, za, zb);
        float v;
        if (g == 0) v = fminf(fmaxf(za * gain * (float)(de.x2 & 1u) + e0[c], -4.0f), 4.0f);      // smirk_trainer.py:208-211
        else if (g == 1) v = gain * es[c];                                                        // :215
        else if (g == 2) v = c < a.num_expression ? gain * tp[c] : e0[c];                         // :220-222
        else v = 0.0f;                                                                            // :238
        a.o_expr[(size_t)r * a.E + c] = v + noise * zb;                                           // :211,216,223,239
    }

    if (lane < 3) {                                    // smirk_trainer.py:226-228, group 3: :241
        const AugDraw dj = aug_philox(row_ctr + 2, AUG_STREAM_ROW, a.seed);
        float zc, zs;
        aug_normal2(lane == 2 ? dj.x2 : dj.x0, lane == 2 ? dj.x3 : dj.x1, zc, zs);
        const float n = lane == 1 ? zs : zc;
        float v = a.jaw[b * 3 + lane] + n * 0.2f * (lane == 0 ? 1.0f : 0.1f) * (float)(ds.x2 & 1u);
        if (lane == 0) v = fminf(fmaxf(v, 0.0f), 0.5f);
        a.o_jaw[r * 3 + lane] = g == 3 ? 0.0f : v;
    }
    if (lane < 2) {                                    // smirk_trainer.py:231-233, group 3: :242
        const AugDraw dl = aug_philox(row_ctr + 3, AUG_STREAM_ROW, a.seed);
        float v = a.eyelid[b * 2 + lane];
        if (a.use_eyelids) v = fminf(fmaxf(v + 0.25f * (2.0f * aug_u01(lane == 0 ? dl.x0 : dl.x1) - 1.0f), 0.0f), 1.0f);
        a.o_eyelid[r * 2 + lane] = g == 3 ? aug_u01(lane == 0 ? dl.x2 : dl.x3) : v;
    }
    for (int c = lane; c < a.S; c += 64) a.o_shape[(size_t)r * a.S + c] = a.shape[(size_t)b * a.S + c];
    if (lane < 3) {
        a.o_pose[r * 3 + lane] = a.pose[b * 3 + lane];
        a.o_cam[r * 3 + lane] = a.cam[b * 3 + lane];
    }
}

extern "C" size_t smirk_cycle_augment_workspace_bytes(int N) {
    return N > 0 ? smirk_align_up((size_t)N * 8, 256) : 0;                                        // row_at int32[N] + key2_at uint32[N]
}

extern "C" int smirk_cycle_augment(const float* expression, const float* jaw, const float* eyelid, const float* shape, const float* pose, const float* cam,
                                   int B, int E, int S, int Ke, int num_expression, int use_eyelids, const float* templates,
                                   const int32_t* class_offsets, const int32_t* class_offsets_host, int n_classes, uint64_t seed, uint64_t offset,
                                   float* out_expression, float* out_jaw, float* out_eyelid, float* out_shape, float* out_pose, float* out_cam,
                                   int32_t* plan, void* ws, size_t ws_bytes, void* stream) {
    if (!expression || !jaw || !eyelid || !shape || !pose || !cam || !templates || !class_offsets || !class_offsets_host || !out_expression || !out_jaw ||
        !out_eyelid || !out_shape || !out_pose || !out_cam || !plan || !ws)
        return SMIRK_ERR_BAD_ARG;
    if (B < 1 || Ke < 1 || E < 1 || S < 1 || num_expression < 1 || num_expression > E || n_classes < 1) return SMIRK_ERR_BAD_ARG;
    if (class_offsets_host[0] != 0) return SMIRK_ERR_BAD_ARG;
    for (int c = 0; c < n_classes; ++c)
        if (class_offsets_host[c + 1] <= class_offsets_host[c]) return SMIRK_ERR_BAD_ARG;         // an empty class cannot be drawn from
    const long long rows = (long long)Ke * B;
    if (rows > SMIRK_AUGMENT_MAX_ROWS) return SMIRK_ERR_UNSUPPORTED;
    const int N = (int)rows;
    if (ws_bytes < smirk_cycle_augment_workspace_bytes(N)) return SMIRK_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* row_at = (int32_t*)ws;
    uint32_t* key2_at = (uint32_t*)ws + N;
    SMIRK_LAUNCH(augment_plan_kernel, dim3((unsigned)((N + AUG_BLOCK - 1) / AUG_BLOCK)), dim3(AUG_BLOCK), 0, st, N, n_classes, class_offsets, seed, offset,
                 plan, row_at, key2_at);
    AugArgs a;
    a.expr = expression; a.jaw = jaw; a.eyelid = eyelid; a.shape = shape; a.pose = pose; a.cam = cam; a.templates = templates;
    a.o_expr = out_expression; a.o_jaw = out_jaw; a.o_eyelid = out_eyelid; a.o_shape = out_shape; a.o_pose = out_pose; a.o_cam = out_cam;
    a.plan = plan; a.row_at = row_at; a.key2_at = key2_at; a.seed = seed; a.offset = offset;
    a.B = B; a.N = N; a.E = E; a.S = S; a.num_expression = num_expression; a.use_eyelids = use_eyelids;
    SMIRK_LAUNCH(augment_apply_kernel, dim3((unsigned)((N + AUG_BLOCK / 64 - 1) / (AUG_BLOCK / 64))), dim3(AUG_BLOCK), 0, st, a);
    return smirk_launch_status();
}
