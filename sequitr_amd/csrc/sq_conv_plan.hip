// Launch plans of the implicit-GEMM convolutions: the channel-block width, the input-channel chunk, the number of channel blocks
// and the split-K factor a call would launch with, as plain host functions.  The launchers of sq_conv_bf16.hip,
// sq_conv_f32_v2.hip and sq_conv_f32_l0.hip take their choices from here; sq_conv_plan reports the same choices without a HIP
// call, so that the CPU suite can pin the plans of the real workloads and check that the kernel tests reach every one.
// sq_conv_walk_plan does the same for the persistent grids of the f32 inference kernels (the level-0 and generic convs, the
// transpose conv): the grid and how many tiles a block walks, from the helpers launch_l0 / launch_v2 / launch_ct call.
#include "sq_conv_epi.h"
#include <stdlib.h>

namespace {
constexpr int TILE = 16;                                        // pixel tiles of 16 x 16 in both families
int64_t ntiles_of(int N, int H, int W) { return (int64_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE) * N; }
}  // namespace

int sq_plan_bf16_kc(int Cin) { return Cin % 32 == 0 ? 32 : (Cin % 16 == 0 ? 16 : 8); }

int sq_plan_bf16_bn(int64_t ntiles, int Cout, bool pn, bool mos) {
    // FORM_PN: every channel of a pixel in one block -- the narrowest width that holds Cout (<= 64)
    if (pn) return Cout <= 16 ? 16 : (Cout <= 32 ? 32 : 64);
    // narrow the channel block until the launch has ~2 blocks per CU (as the f32 v2 family): the GAN's 4x4 .. 32x32
    // levels are a handful of mosaic tiles x 512 .. 64 channels, and 64-channel blocks leave most of the chip idle
    int bn = Cout >= 64 ? 64 : (Cout > 16 ? 32 : 16);
    static const int narrow = [] { const char *e = getenv("SQ_CONV_BF16_NARROW"); return e ? atoi(e) : 1; }();
    while (narrow && bn > 16 && ntiles * ((Cout + bn - 1) / bn) < 2 * 256) bn >>= 1;
    static const int force_bn = [] { const char *e = getenv("SQ_MOS_BN"); return e ? atoi(e) : 0; }();   // experiment switch: block width of the mosaic launches
    if (mos && (force_bn == 16 || force_bn == 32 || force_bn == 64) && force_bn <= ((Cout + 15) / 16) * 16) bn = force_bn;
    return bn;
}

int sq_plan_mosaic_splitk(int Nimg, int h, int w, int Cin, int Cout, int R, int Cc, bool have_ws, int64_t workspace_bytes) {
    // blocks the unsplit launch would have (16-channel blocks once narrowed) vs the chip
    const int H = R * (h + 1), W = Cc * (w + 1);
    const int nchunk = Cin / sq_plan_bf16_kc(Cin);
    const int64_t blocks = ntiles_of(1, H, W) * ((Cout + 15) / 16);
    const int64_t slice = (int64_t)Nimg * h * w * Cout * 4;
    int S = 1;
    static const int sk_on = [] { const char *e = getenv("SQ_CONV_SPLITK"); return e ? atoi(e) : 1; }();
    if (sk_on && have_ws && Cout % 4 == 0 && blocks < 256 && nchunk >= 4)
        while (S < 8 && nchunk % (2 * S) == 0 && nchunk / (2 * S) >= 2 && blocks * S < 512 && slice * 2 * S <= workspace_bytes) S *= 2;
    static const int force_s = [] { const char *e = getenv("SQ_MOS_S"); return e ? atoi(e) : 0; }();   // experiment switch (tools/r04_mosaic_sweep.py)
    if (force_s >= 1 && have_ws && nchunk % force_s == 0 && slice * force_s <= workspace_bytes) S = force_s;
    return S;
}

int sq_plan_f32_bn(int64_t ntiles, int Cout) {
    // widest channel block the layer fills the chip with: small images (GAN 4x4..32x32 levels, small batches) have few pixel
    // tiles, so trade operand reuse for blocks until there are ~2 per CU.  BN only changes which block computes an output,
    // never its fmaf chain.  (32-channel blocks for the wide layers, three blocks per CU: 5.189 vs 5.107 ms per step -- 64 it stays)
    int bn = Cout >= 64 ? 64 : (Cout > 16 ? 32 : 16);
    while (bn > 16 && ntiles * ((Cout + bn - 1) / bn) < 2 * 256) bn >>= 1;
    return bn;
}

bool sq_plan_f32_stage32(int bn, int KS, int KC, int Cin, bool concat) {
    // 32 -> 32 (and wider-input) 3x3 layers on 32-channel blocks: stage 32 input channels per item (same chain)
    // SQ_CONV_STAGE32=0: A/B switch back to 16-channel items
    static const bool on = [] { const char *e = getenv("SQ_CONV_STAGE32"); return !(e && e[0] == '0'); }();
    return KS == 3 && KC == 16 && bn == 32 && Cin % 32 == 0 && !concat && on;
}

bool sq_plan_l0_takes(int mode, int cout, int act, int H, int W, bool concat, int head_c, bool pooled) {
    if (cout != 16 && !(cout == 32 && mode == 0 && !head_c && !pooled)) return false;
    const char *e = getenv("SQ_CONV_L0");                       // SQ_CONV_L0=0: A/B switch back to the generic kernel; read per
    if (e && e[0] == '0') return false;                         // call: the parity tests flip it in-process
    if (act != SQ_ACT_RELU || H % 16 != 0 || W % 16 != 0 || concat) return false;
    if (head_c && head_c != 2) return false;
    if (head_c && pooled) return false;
    return true;
}

bool sq_plan_r32_takes(int N, int H, int W, int Cin, int Cout, int K, int act, bool wscale1, bool concat, bool head, bool pooled) {
    // the 32 -> 32 ReLU layers on whole 16 x 16 tiles, where the plan is the generic kernel's 32-channel block with 32 staged
    // channels (<32,3,32,0>: ntiles >= 512); the kernel walks that form's grid.  Both epilogues (plain, pooled) are on
    (void)pooled;
    if (K != 3 || Cin != 32 || Cout != 32 || !wscale1 || act != SQ_ACT_RELU || concat || head) return false;
    if (N <= 0 || H <= 0 || W <= 0 || H % 16 != 0 || W % 16 != 0) return false;
    const char *e = getenv("SQ_CONV_R32");                      // SQ_CONV_R32=0: A/B switch back to the generic kernel; read per
    if (e && e[0] == '0') return false;                         // call: the parity tests flip it in-process
    if ((size_t)N * H * W * 32 * 4 >= ((size_t)1 << 31)) return false;
    const int bn = sq_plan_f32_bn(ntiles_of(N, H, W), Cout);
    return bn == 32 && sq_plan_f32_stage32(bn, K, 16, Cin, concat);
}

// host-only query of the rule above for the plain (pooled = 0) and pooled entry points at wscale == 1
extern "C" int sq_conv_r32_takes_f32(int N, int H, int W, int Cin, int Cout, int K, int act, int pooled) {
    return sq_plan_r32_takes(N, H, W, Cin, Cout, K, act, true, false, false, pooled != 0) ? 1 : 0;
}

int sq_plan_l0_grid(int ntiles, int occ) {
    const int want = 256 * occ;
    return ntiles < want ? ntiles : want;
}

void sq_plan_tile_stride(int G, int tiles_x, int tiles_y, int *gx, int *gy, int *gn) {
    const int per_image = tiles_x * tiles_y;
    *gn = G / per_image;
    *gy = (G % per_image) / tiles_x;
    *gx = (G % per_image) % tiles_x;
}

int sq_plan_v2_grid(int ntiles, int cblocks, int occ, int *tiles_per_block) {
    int want = (256 * occ + cblocks - 1) / cblocks;
    if (want < 1) want = 1;
    int tpb = (ntiles + want - 1) / want;
    if (tpb < 1) tpb = 1;
    *tiles_per_block = tpb;
    return (ntiles + tpb - 1) / tpb;
}

int sq_plan_ct_wni() {
    static const int wni = [] { const char *v = getenv("SQ_CONVT_WNI"); return v ? atoi(v) : SQ_CT_WNI; }();   // read once per process
    return wni == 4 || wni == 1 ? wni : 2;
}

bool sq_plan_ct_takes(int N, int H, int W, int Cin, int Cout) {
    const char *e = getenv("SQ_CONVT_V2");                          // SQ_CONVT_V2=0: A/B switch back to the 64 x 64 kernel
    if (e && e[0] == '0') return false;
    const size_t P = (size_t)N * H * W;
    if (Cin % 32 != 0 || Cout % 32 != 0) return false;
    if (P * 4 * Cout * 4 >= ((size_t)1 << 31) || P * Cin * 4 >= ((size_t)1 << 31)) return false;
    return true;
}

int sq_plan_ct_grid(int total, int mtiles, int occ) {
    const int want = 256 * occ;
    int G = total < want ? total : want;
    if (G > mtiles) G -= G % mtiles;                                // the row tiles of one pixel tile start together
    return G;
}

// The walk of the persistent f32 inference kernels: which kernel takes the call, its grid, and how many items the busiest and the
// idlest block take (block b takes item b, b + G, ...: ceil and floor of items / G).  The dispatch conditions are those of the
// entry points (sq_conv_mfma_v2, sq_conv3x3_pool_fwd_f32, ..., sq_convT_v2_launch); the grids come from the launchers' helpers.
extern "C" int sq_conv_walk_plan(int form, int N, int H, int W, int Cin, int Cout, int K, int act, int flags, int head_c,
                                 int *out) {
    SQ_REQUIRE(out, "sq_conv_walk_plan: null out");
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "sq_conv_walk_plan: bad shape");
    SQ_REQUIRE(act >= SQ_ACT_NONE && act <= SQ_ACT_LEAKY, "sq_conv_walk_plan: bad activation %d", act);
    for (int i = 0; i < SQ_WALK_N; ++i) out[i] = 0;
    if (form == SQ_PLAN_CONVT) {                                    // (N, H, W): the low-resolution input
        if (!sq_plan_ct_takes(N, H, W, Cin, Cout)) return SQ_OK;    // SQ_WALK_NONE: the 64 x 64 kernel, no walk
        const int wni = sq_plan_ct_wni();
        const int mtiles = 4 * Cout / SQ_CT_BM, ntiles = (N * H * W + 32 * wni - 1) / (32 * wni);
        const int total = mtiles * ntiles, G = sq_plan_ct_grid(total, mtiles, sq_ct_occ(wni));
        out[SQ_WALK_KERNEL] = SQ_WALK_CONVT;
        out[SQ_WALK_G] = G;
        out[SQ_WALK_TMIN] = total / G;
        out[SQ_WALK_TMAX] = (total + G - 1) / G;
        out[SQ_WALK_MTILES] = mtiles;
        out[SQ_WALK_CBLOCKS] = 1;
        out[SQ_WALK_ITEMS] = total;
        out[SQ_WALK_TILEPX] = 32 * wni;
        return SQ_OK;
    }
    const bool pooled = form == SQ_PLAN_POOL || (form == SQ_PLAN_FIRSTBLOCK && (flags & SQ_PLAN_POOLED));
    SQ_REQUIRE(!pooled || (H % 2 == 0 && W % 2 == 0), "sq_conv_walk_plan: pooling needs even H, W");
    int mode = 0, bn = 16, kc = 16;                                 // of the generic kernel's instantiation
    bool offer = false;                                             // the entry point asks the level-0 kernel first
    switch (form) {
    case SQ_PLAN_PLAIN:
        SQ_REQUIRE((K == 1 || K == 3) && Cout % 4 == 0 && (Cin % 16 == 0 || Cin == 8),
                   "sq_conv_walk_plan: the f32 v2 kernels take Cin %% 16 == 0 (or 8), Cout %% 4 == 0");
        offer = Cin == 16 && (Cout == 16 || Cout == 32) && K == 3 && !(flags & SQ_PLAN_WSCALE);
        break;
    case SQ_PLAN_POOL:
        SQ_REQUIRE(K == 3 && Cin % 16 == 0 && Cout % 4 == 0, "sq_conv_walk_plan: the pooled form is 3x3, Cin %% 16 == 0, Cout %% 4 == 0");
        offer = Cin == 16 && Cout == 16;
        break;
    case SQ_PLAN_CONCAT:
        SQ_REQUIRE((K == 1 || K == 3) && Cin % 32 == 0 && Cout % 4 == 0, "sq_conv_walk_plan: concat takes Cin = 2 Ca, Ca %% 16 == 0");
        break;
    case SQ_PLAN_FIRSTBLOCK:
        SQ_REQUIRE(K == 3 && Cin == 1 && Cout == 16 && act == SQ_ACT_RELU, "sq_conv_walk_plan: the first block is 1 -> 16 -> 16, ReLU");
        offer = true;
        mode = 1;
        break;
    case SQ_PLAN_UP:                                                // (N, H, W): the output
        SQ_REQUIRE(K == 3 && Cin == 16 && Cout == 16 && H % 2 == 0 && W % 2 == 0, "sq_conv_walk_plan: the up block is 16 -> 16 at even H, W");
        offer = true;
        mode = 2;
        break;
    case SQ_PLAN_HEAD:
        SQ_REQUIRE(K == 3 && Cin % 16 == 0 && Cout == 16 && head_c >= 1 && head_c <= 4, "sq_conv_walk_plan: the head is Cin -> 16 -> head_c (1..4)");
        offer = Cin == 16;
        break;
    default:
        SQ_REQUIRE(false, "sq_conv_walk_plan: form %d has no persistent f32 kernel", form);
    }
    SQ_REQUIRE((size_t)N * H * W * (size_t)(Cin > Cout ? Cin : Cout) * 4 < ((size_t)1 << 31), "sq_conv_walk_plan: tensors must be < 2 GiB");
    const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE, ntiles = (int)ntiles_of(N, H, W);
    int G, cblocks = 1;
    if (offer && sq_plan_l0_takes(mode, Cout, act, H, W, false, form == SQ_PLAN_HEAD ? head_c : 0, pooled)) {
        out[SQ_WALK_KERNEL] = SQ_WALK_L0;
        G = sq_plan_l0_grid(ntiles, sq_l0_occ(mode == 2, Cout / 16));
    } else {
        if (form == SQ_PLAN_PLAIN || form == SQ_PLAN_POOL || form == SQ_PLAN_CONCAT) {   // dispatch_bn
            kc = Cin % 16 == 0 ? 16 : 8;
            bn = sq_plan_f32_bn(ntiles, Cout);
            if (sq_plan_f32_stage32(bn, K, kc, Cin, form == SQ_PLAN_CONCAT)) kc = 32;
        }
        cblocks = (Cout + bn - 1) / bn;
        int tpb;
        out[SQ_WALK_KERNEL] = SQ_WALK_V2;
        G = sq_plan_v2_grid(ntiles, cblocks, sq_v2_occ(bn, kc, mode == 2), &tpb);
    }
    out[SQ_WALK_G] = G;
    out[SQ_WALK_TMIN] = ntiles / G;
    out[SQ_WALK_TMAX] = (ntiles + G - 1) / G;
    sq_plan_tile_stride(G, tiles_x, tiles_y, &out[SQ_WALK_GX], &out[SQ_WALK_GY], &out[SQ_WALK_GN]);
    out[SQ_WALK_CBLOCKS] = cblocks;
    out[SQ_WALK_ITEMS] = ntiles;
    out[SQ_WALK_TILEPX] = TILE * TILE;
    return SQ_OK;
}

extern "C" int sq_conv_plan(int family, int form, int N, int H, int W, int Cin, int Cout, int K, int act, int flags,
                            const int *mosaic, int64_t workspace_bytes, int *out) {
    SQ_REQUIRE(out, "sq_conv_plan: null out");
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && (K == 1 || K == 3), "sq_conv_plan: bad shape / K");
    SQ_REQUIRE(act >= SQ_ACT_NONE && act <= SQ_ACT_LEAKY, "sq_conv_plan: bad activation %d", act);
    out[0] = out[1] = out[2] = 0;
    out[3] = 1;
    out[4] = 0;
    if (family == SQ_PLAN_F32) {
        SQ_REQUIRE(!mosaic, "sq_conv_plan: the f32 family has no mosaic form");
        SQ_REQUIRE(Cout % 4 == 0 && (Cin % 16 == 0 || (Cin == 8 && form == SQ_PLAN_PLAIN)),
                   "sq_conv_plan: the f32 v2 kernels take Cin %% 16 == 0 (or 8, plain), Cout %% 4 == 0");
        SQ_REQUIRE(form == SQ_PLAN_PLAIN || form == SQ_PLAN_CONCAT || (form == SQ_PLAN_POOL && K == 3),
                   "sq_conv_plan: f32 form %d at K=%d does not exist", form, K);
        const bool wscale1 = !(flags & SQ_PLAN_WSCALE);
        // the level-0 kernel: sq_conv_mfma_v2 (plain) and sq_conv3x3_pool_fwd_f32 (pool) offer it the 16-channel layers
        const bool offer = form == SQ_PLAN_PLAIN ? (Cin == 16 && (Cout == 16 || Cout == 32) && K == 3 && wscale1)
                                                 : (form == SQ_PLAN_POOL && Cin == 16 && Cout == 16);
        if (offer && sq_plan_l0_takes(0, Cout, act, H, W, false, 0, form == SQ_PLAN_POOL)) {
            out[0] = Cout;
            out[1] = 16;
            out[2] = 1;
            out[4] = 1;
            return SQ_OK;
        }
        const int KC = Cin % 16 == 0 ? 16 : 8;
        const int bn = sq_plan_f32_bn(ntiles_of(N, H, W), Cout);
        const bool s32 = sq_plan_f32_stage32(bn, K, KC, Cin, form == SQ_PLAN_CONCAT);
        out[0] = bn;
        out[1] = s32 ? 32 : KC;
        out[2] = (Cout + bn - 1) / bn;
        return SQ_OK;
    }
    SQ_REQUIRE(family == SQ_PLAN_BF16 || family == SQ_PLAN_MIXED, "sq_conv_plan: bad family %d", family);
    SQ_REQUIRE(Cin % 8 == 0 && Cout % 4 == 0, "sq_conv_plan: Cin=%d (multiple of 8), Cout=%d (multiple of 4)", Cin, Cout);
    const bool bf = family == SQ_PLAN_BF16;
    int NN = N, HH = H, WW = W;
    if (mosaic) {
        SQ_REQUIRE(K == 3 && (form == SQ_PLAN_PLAIN || form == SQ_PLAN_ACTGATE), "sq_conv_plan: the mosaic forms are 3x3 plain / act-gated");
        SQ_REQUIRE(mosaic[0] > 0 && mosaic[1] > 0 && (int64_t)mosaic[0] * mosaic[1] >= N && H <= 8 && W <= 8,
                   "sq_conv_plan: mosaic of R x Cc >= Nimg cells of images up to 8 x 8");
        NN = 1;
        HH = mosaic[0] * (H + 1);
        WW = mosaic[1] * (W + 1);
        if (bf) out[3] = sq_plan_mosaic_splitk(N, H, W, Cin, Cout, mosaic[0], mosaic[1], workspace_bytes > 0, workspace_bytes);
    } else {
        switch (form) {
        case SQ_PLAN_PLAIN: case SQ_PLAN_ACTGATE: break;
        case SQ_PLAN_POOL: case SQ_PLAN_JUNCTION:
            SQ_REQUIRE(bf && K == 3, "sq_conv_plan: form %d is a 3x3 form on bf16 tensors", form); break;
        case SQ_PLAN_MASK: case SQ_PLAN_MASKGATE:
            SQ_REQUIRE(bf && K == 3 && Cout % 16 == 0, "sq_conv_plan: the mask forms are 3x3, Cout %% 16 == 0, bf16 tensors"); break;
        case SQ_PLAN_PIXELNORM:
            SQ_REQUIRE(bf && K == 3 && Cout % 8 == 0 && Cout <= 64, "sq_conv_plan: the pixel-norm form is 3x3, Cout %% 8 == 0, <= 64"); break;
        case SQ_PLAN_FIRSTBLOCK:
            SQ_REQUIRE(bf && K == 3 && Cin == 16 && Cout == 16, "sq_conv_plan: the first block is the 3x3 16 -> 16 conv"); break;
        default:
            SQ_REQUIRE(false, "sq_conv_plan: form %d does not exist in family %d", form, family);
        }
    }
    const int bn = sq_plan_bf16_bn(ntiles_of(NN, HH, WW), Cout, form == SQ_PLAN_PIXELNORM, mosaic != nullptr);
    out[0] = bn;
    out[1] = sq_plan_bf16_kc(Cin);
    out[2] = (Cout + bn - 1) / bn;
    return SQ_OK;
}
