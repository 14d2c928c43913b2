// tiles.h -- what every conv tile id (smap_op.tile) means, written down ONCE for the C side (internal, not part of the C ABI).
// The Python side keeps the same rows in TILE_TABLE at the top of smap_amd/engine.py; tests/test_host_cpu.py compares the two
// fact by fact through smap_conv_tile_dims / _bk / _tail_bn and through what smap_plan_create accepts.
//
// Adding a tile id: one row here, one row in engine.py, one `case` in the launch switch of the family's file.  The launch
// helpers take the id as a template argument and read BM / BN / BK / the tail chunk from the row, and they static_assert the
// family and the capability they instantiate, so a dispatch line that disagrees with its row does not build.
#pragma once

enum TileFamily {
    TF_IGEMM,      // conv.hip: implicit GEMM, LDS-staged (or register) epilogue
    TF_HALO,       // conv3.hip: halo-tiled plain 3x3 stride-1
    TF_PERSIST,    // convp.hip: persistent workgroups with loader waves, register epilogue (no fused bilinear add, no fp32 output)
    TF_TAIL,       // convf.hip: a Bottleneck's 3x3 (BN = all of its planes) with the following 1x1 fused in
    TF_BLOCK       // convb.hip / convc.hip: a whole Bottleneck (1x1 -> 3x3 -> 1x1 + residual) per pixel tile, split precision only
};

enum TileCap : unsigned {      // which instances of its kernel a tile id has
    TC_F16 = 1,                // an fp16 instance (smap_op.precision = 0)
    TC_X3 = 2,                 // a split-precision instance (precision = 1)
    TC_BOTH = TC_F16 | TC_X3,
    // conv.hip's kernel beyond the plain instance, in every precision the tile has:
    TC_SPLITK = 4,             // split K (smap_op.ksplit > 1)
    TC_DUAL = 8,               // second input concatenated along K (smap_op.in2_C > 0)
    TC_RELUSUM = 16,           // relu(conv) + relu(conv) (smap_op.in2_mode = 1)
    TC_REGEPI = 32,            // register epilogue INSTEAD of the LDS-staged one: fp16 outputs, residual + ReLU only
    TC_TAPDOT = 64             // tap-dot epilogue (smap_op.tap_n = 9): one N tile of 256 channels
};

struct TileRow {
    int id;
    TileFamily family;
    int bm, bn;                // output tile: pixels x channels
    int bk16, bkx3;            // halves per staged K tile (= the packing unit of the weights) in fp16 / split precision
    int tail_bn;               // channels per chunk of the fused 1x1 tail (TF_TAIL, TF_BLOCK), else 0
    int planes;                // TF_BLOCK: planes of the Bottleneck (its output has 4 x planes channels), else 0
    bool first;                // TF_BLOCK: a layer's FIRST block (planes input channels, 1x1 shortcut conv instead of + x)
    unsigned caps;
};

// The halo kernels' LDS rows are always 128 bytes: 64 channels, or [hi32 | lo32] of 32 channels in split precision.
constexpr TileRow SMAP_TILES[] = {
    // 0..4: two-stage (double-buffered) pipelines of 64-half K tiles: half the barriers per K of the BK = 32 tiles
    {0, TF_IGEMM, 128, 128, 64, 64, 0, 0, false, TC_BOTH},                              // x3: 128 KiB
    {1, TF_IGEMM, 128, 64, 64, 64, 0, 0, false, TC_BOTH},                               // x3: 96 KiB
    {2, TF_IGEMM, 64, 64, 64, 64, 0, 0, false, TC_BOTH | TC_SPLITK},                        // x3: 64 KiB
    {3, TF_IGEMM, 128, 32, 64, 64, 0, 0, false, TC_BOTH},                               // x3: 80 KiB; the Cout <= 32 heads
    {4, TF_IGEMM, 64, 128, 64, 64, 0, 0, false, TC_BOTH},                               // x3: 96 KiB
    // 5..9: the same tiles with deeper LDS-DMA pipelines (fp16; 7 also in split precision)
    {5, TF_IGEMM, 128, 128, 64, 32, 0, 0, false, TC_F16},                               // 128 KiB LDS, 1 block/CU, 3 tiles in flight
    {6, TF_IGEMM, 128, 64, 64, 32, 0, 0, false, TC_F16},                                //  72 KiB, 2 blocks/CU
    // 7 in split precision: 128 KiB, THREE 64-half K tiles in flight (the small grids of batch-1 schedules leave the LDS of a CU to one
    // workgroup anyway; their K loops are bound by the latency of the one tile a two-stage pipeline keeps in flight)
    {7, TF_IGEMM, 64, 64, 64, 64, 0, 0, false, TC_BOTH | TC_SPLITK},                        //  64 KiB, 2 blocks/CU
    {8, TF_IGEMM, 128, 32, 64, 32, 0, 0, false, TC_F16},                                //  60 KiB, 2 blocks/CU
    {9, TF_IGEMM, 64, 128, 64, 32, 0, 0, false, TC_F16},                                //  72 KiB, 2 blocks/CU
    // (10..18 belonged to a register-epilogue GEMM that no measured table entry selected: tools/experiments/)
    // 20..27: BK = 32 staging (smaller LDS, more workgroups per CU); LDS-staged epilogue kept.  LDS fp16 / x3:
    {20, TF_IGEMM, 128, 128, 32, 32, 0, 0, false, TC_BOTH | TC_SPLITK | TC_DUAL},           // 64 KiB (the fp32 epilogue tile) / 64 KiB
    {21, TF_IGEMM, 128, 64, 32, 32, 0, 0, false, TC_BOTH},                              // 32 / 48 KiB
    {22, TF_IGEMM, 64, 64, 32, 32, 0, 0, false, TC_BOTH | TC_SPLITK},                       // 16 / 32 KiB
    {23, TF_IGEMM, 64, 128, 32, 32, 0, 0, false, TC_BOTH},                              // 32 / 48 KiB
    {24, TF_IGEMM, 128, 128, 32, 32, 0, 0, false, TC_BOTH},                             // 64 KiB, 3 tiles in flight / 96 KiB, 2 (x3 is 3-stage)
    {25, TF_IGEMM, 128, 64, 32, 32, 0, 0, false, TC_BOTH},                              // 36 / 72 KiB, 2 tiles in flight
    {26, TF_IGEMM, 64, 64, 32, 32, 0, 0, false, TC_BOTH},                               // 32 / 64 KiB, 3 tiles in flight
    {27, TF_IGEMM, 64, 128, 32, 32, 0, 0, false, TC_BOTH},                              // 36 / 72 KiB
    // 30..39: halo-tiled 3x3, four waves, BM = 128 output pixels as an 8x16 / 4x32 patch
    {30, TF_HALO, 128, 64, 64, 32, 0, 0, false, TC_BOTH},                               //  64 KiB LDS
    {31, TF_HALO, 128, 128, 64, 32, 0, 0, false, TC_BOTH},                              //  80 KiB
    {32, TF_HALO, 128, 64, 64, 32, 0, 0, false, TC_BOTH},                               //  72 KiB
    {33, TF_HALO, 128, 128, 64, 32, 0, 0, false, TC_BOTH},                              //  88 KiB
    {34, TF_HALO, 128, 64, 64, 32, 0, 0, false, TC_BOTH},                               //  80 KiB: 30 with three weight tiles in flight
    {35, TF_HALO, 128, 128, 64, 32, 0, 0, false, TC_BOTH},                              //  96 KiB: 31 with two
    {36, TF_HALO, 128, 64, 64, 32, 0, 0, false, TC_BOTH},                               //  80 KiB: 32 with two
    {37, TF_HALO, 128, 128, 64, 32, 0, 0, false, TC_BOTH},                              // 104 KiB: 33 with two
    {38, TF_HALO, 128, 32, 64, 32, 0, 0, false, TC_BOTH},                               //  64 KiB: Cout <= 32 heads, 4 x 1 waves
    {39, TF_HALO, 128, 32, 64, 32, 0, 0, false, TC_BOTH},                               //  72 KiB
    // 40..45: the same kernel with EIGHT waves
    {40, TF_HALO, 128, 128, 64, 32, 0, 0, false, TC_BOTH},    //  80 KiB: 8x16 pixels, waves of 32 px x 64 ch, two workgroups per CU (64 x 32 waves spill at 128 VGPRs)
    {41, TF_HALO, 256, 128, 64, 32, 0, 0, false, TC_BOTH},    // 144 KiB: 16x16 pixels, waves of 64 x 64, two weight tiles in flight
    {42, TF_HALO, 256, 64, 64, 32, 0, 0, false, TC_BOTH},     // 128 KiB: 16x16 pixels x 64 channels (the 43-channel heads), waves of 64 x 32
    {43, TF_HALO, 256, 128, 64, 32, 0, 0, false, TC_BOTH},    // 144 KiB: 8x32 pixels
    {44, TF_HALO, 256, 128, 64, 32, 0, 0, false, TC_BOTH},    // 41 with the two waves of a SIMD half an iteration apart
    {45, TF_HALO, 256, 128, 64, 32, 0, 0, false, TC_BOTH},    // 43, staggered
    // 50..55: conv.hip with EIGHT waves per workgroup (two per SIMD from one workgroup: the low-resolution layers).  The relu-sum instances
    // exist on these only: the four-wave 128 x 128 instance needs 288 registers (one wave per SIMD)
    {50, TF_IGEMM, 128, 128, 32, 32, 0, 0, false, TC_BOTH | TC_DUAL | TC_RELUSUM},          // 64 KiB, waves of 64x32
    {51, TF_IGEMM, 128, 128, 32, 32, 0, 0, false, TC_BOTH | TC_DUAL | TC_RELUSUM},          // 64 KiB, waves of 32x64
    {52, TF_IGEMM, 128, 128, 64, 64, 0, 0, false, TC_BOTH},                             // x3: 128 KiB, BK = 64
    {53, TF_IGEMM, 256, 128, 32, 32, 0, 0, false, TC_BOTH | TC_DUAL | TC_RELUSUM},          // 128 KiB (fp32 epilogue tile) / 96 KiB, waves of 64x64
    {54, TF_IGEMM, 128, 256, 32, 32, 0, 0, false, TC_BOTH | TC_DUAL | TC_RELUSUM | TC_TAPDOT},   // x3: 96 KiB, waves of 64x64
    {55, TF_IGEMM, 128, 128, 32, 32, 0, 0, false, TC_BOTH},   // 4-stage pipeline, 3 K tiles in flight (bytes in flight, not occupancy, for the streaming layers): 64 / 128 KiB
    // 56: 256 x 256, eight waves of 128 x 64, two 64 KiB LDS stages leave no room for a staging tile: half the L2 -> LDS bytes per MFMA of
    // the 128 x 128 tiles.  Split precision only
    {56, TF_IGEMM, 256, 256, 64, 32, 0, 0, false, TC_X3 | TC_REGEPI},
    // 60..65: persistent workgroups.  LDS stages fp16 / x3.  (66, 68, 69, 70 -- split loaders, 64-half K tiles, eight loader waves -- were
    // experiments that no measured table entry selects; the template parameters NLA / P_BK / P_NLW they instantiated remain)
    {60, TF_PERSIST, 128, 256, 32, 32, 0, 0, false, TC_BOTH},                           // 8 compute waves of 64 px x 64 ch; 4 x 24 / 3 x 48 KiB
    {61, TF_PERSIST, 256, 128, 32, 32, 0, 0, false, TC_BOTH},                           // 4 x 24 / 3 x 48 KiB
    {62, TF_PERSIST, 128, 128, 32, 32, 0, 0, false, TC_BOTH},                           // 8 compute waves of 32 px x 64 ch; 4 x 16 / 4 x 32 KiB
    {63, TF_PERSIST, 128, 64, 32, 32, 0, 0, false, TC_BOTH},                            // six stages (x3: 6 x 24 KiB)
    {64, TF_PERSIST, 128, 64, 32, 32, 0, 0, false, TC_BOTH},                            // three
    {65, TF_PERSIST, 128, 64, 32, 32, 0, 0, false, TC_BOTH},                            // two
    // 80..82: 3x3 (all BN = planes output channels in one tile) + the 1x1 tail in chunks of tail_bn channels
    {80, TF_TAIL, 128, 64, 64, 32, 64, 0, false, TC_BOTH},                              // 80 KiB both phases: two workgroups per CU
    {81, TF_TAIL, 128, 64, 64, 32, 128, 0, false, TC_BOTH},                             // 96 KiB
    {82, TF_TAIL, 128, 128, 64, 32, 64, 0, false, TC_BOTH},                             // 128 KiB
    // 90..94: a whole Bottleneck; BM = output pixels per workgroup, BN = planes
    {90, TF_BLOCK, 64, 64, 64, 32, 64, 64, false, TC_X3},                              // 4 x 16 pixel tiles
    {91, TF_BLOCK, 128, 64, 64, 32, 64, 64, false, TC_X3},                             // 8 x 16
    {92, TF_BLOCK, 64, 64, 64, 32, 64, 64, true, TC_X3},                               // first block of layer1, 4 x 16
    {93, TF_BLOCK, 128, 64, 64, 32, 64, 64, true, TC_X3},                              //   8 x 16
    {94, TF_BLOCK, 128, 128, 64, 32, 128, 128, false, TC_X3},                          // convc.hip: 128 planes / 512 channels (layer2), 8 x 16, eight waves
};

constexpr int SMAP_N_TILES = sizeof(SMAP_TILES) / sizeof(SMAP_TILES[0]);

// the row of a tile id, or null
constexpr const TileRow* tile_find(int id)
{
    for (int i = 0; i < SMAP_N_TILES; ++i)
        if (SMAP_TILES[i].id == id) return &SMAP_TILES[i];
    return nullptr;
}

// the same as a constant expression (template arguments of the launch helpers); an id without a row does not compile
constexpr TileRow tile_row(int id) { return *tile_find(id); }

constexpr int tile_bk(const TileRow& t, bool x3) { return x3 ? t.bkx3 : t.bk16; }
constexpr bool tile_has(const TileRow& t, bool x3, unsigned caps = 0) { return (t.caps & ((x3 ? TC_X3 : TC_F16) | caps)) == ((x3 ? TC_X3 : TC_F16) | caps); }
