/* smirk_mica.h — extension table of libsmirk_hip.so for the pre-training shape term: the frozen MICA network
 *   ArcFace (iresnet100) -> F.normalize -> MappingNetwork      (reference: src/models/MICA/mica.py:48-94, arcface.py:32-198)
 *
 * The convolutions of the network are the entries of smirk_hip.h (smirk_conv_igemm_f16x3 with BatchNorm as the epilogue's scale / shift); this header
 * declares everything around them.  It is versioned on its own (smirk_mica_abi_version): the main table of smirk_hip.h and its version do not move when
 * an entry is added here.  The conventions are those of smirk_hip.h: device pointers, caller-owned buffers, work enqueued on `stream`, 0 = SMIRK_OK.
 * Every pointer to a split16 tensor, a workspace or a weight matrix must be 16-byte aligned; NULL, a misaligned pointer, a channel count that is no
 * multiple of 8 and non-positive sizes return SMIRK_ERR_BAD_ARG before the device is touched, a tensor of 2 GiB or more SMIRK_ERR_UNSUPPORTED.
 * No entry uses float atomics: every sum has a fixed order that depends on the shapes alone, so two runs agree bit for bit.
 */
#ifndef SMIRK_MICA_H
#define SMIRK_MICA_H

#include "smirk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMIRK_MICA_ABI_VERSION 1
#define SMIRK_MICA_FC_MAX_B 64      /* rows of one fully connected call */
#define SMIRK_MICA_HEAD_LAYERS 5    /* four hidden Linear + leaky_relu(0.2), one output Linear */
#define SMIRK_MICA_HEAD_MAX_DIM 1024 /* widest layer the head kernel keeps in LDS */

int smirk_mica_abi_version(void);

/* mica.py:70-71: v = (img - 0.5) / 0.5 with the channels reordered [2, 1, 0]; img [B][3][H][W] fp32 -> out [B][H][W][8] split16, channels 3..7 zero.
 * The inputs come from outside the library: a non-finite pixel (or |v| >= 65520) sets the range flag. */
int smirk_mica_prepare_split16(const float* img, void* out, int B, int H, int W, void* stream);

/* z = in * scale[c] + shift[c]; out = z > 0 ? z : slope[c] * z over a split16 tensor [M][C] (BatchNorm in eval mode and / or PReLU, arcface.py:53,56).
 * scale, shift and slope are fp32 [C], each nullable (1 / 0 / the identity).  out == in is allowed. */
int smirk_mica_affine_prelu_split16(const void* in, const float* scale, const float* shift, const float* slope, void* out, long long M, int C, void* stream);

/* out[b][n] = bias[n] + sum_k x[b][k] * w[n][k] (arcface.py:196 with bn2, the flatten order and `features` folded into w and bias by the caller):
 * x split16 [B][K], w fp32 [N][K], bias fp32 [N], out fp32 [B][N]; B <= SMIRK_MICA_FC_MAX_B, K % 8 == 0.  K is split across workgroups into fp32
 * partials in `ws` (smirk_mica_fc_workspace_bytes; 0 for arguments the entry refuses), which a second launch adds in split order.  fp32 FMA. */
size_t smirk_mica_fc_workspace_bytes(int B, int K, int N);
int smirk_mica_fc_split16(const void* x, const float* w, const float* bias, float* out, void* ws, size_t ws_bytes, int B, int K, int N, void* stream);

typedef struct SmirkMicaLinear {
    const float* w;         /* [n_out][n_in] */
    const float* b;         /* [n_out] */
    int32_t n_in, n_out;    /* 1 .. SMIRK_MICA_HEAD_MAX_DIM; n_in of a layer = n_out of the one before */
} SmirkMicaLinear;
typedef struct SmirkMicaHead {
    SmirkMicaLinear layer[SMIRK_MICA_HEAD_LAYERS];
} SmirkMicaHead;

/* mica.py:74-76, 34-43: h = feat / max(|feat|_2, 1e-12); four times h = leaky_relu(W h + b, 0.2); out = W h + b.  feat fp32 [B][layer[0].n_in],
 * out fp32 [B][layer[4].n_out]; `head` is a host struct of device pointers.  One workgroup per row, fp32. */
int smirk_mica_head(const float* feat, const SmirkMicaHead* head, float* out, int B, void* stream);

#ifdef __cplusplus
}
#endif
#endif
