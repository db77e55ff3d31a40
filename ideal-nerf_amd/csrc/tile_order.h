// Which tile a persistent workgroup renders in which round (the colour-gated fp32 kernel).
//
// A grid of G workgroups walks ntiles tiles in rounds of G consecutive tiles.  Plain grid-stride gives workgroup c the tiles
// c, c + G, c + 2G, ...: when a frame's row is a multiple of G tiles, c sees the same columns in every row, and the live tiles
// of a blob in the image pile up on the workgroups under it.  The skewed order rotates every round by kTileSkew places more:
//
//     tile(r, c) = r * G + ((c + r * kTileSkew) mod G),       workgroup c stops at its first tile >= ntiles.
//
// Every round is a bijection of its G tiles, so each tile is rendered once for any ntiles and G; a tile >= ntiles in round r
// means every tile of round r + 1 is out of range as well ((r + 1) * G > tile).  Plain C, no includes: the kernel uses
// tile_order_next (additions, one compare, one select -- all on workgroup-uniform values, so scalar instructions), a host
// program can include the file as it is (tests/test_tile_order_cpu.py, tools/gate_balance_model.py's constant).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IDN_TILE_HD __host__ __device__ static inline
#else
#define IDN_TILE_HD static inline
#endif

// Odd, coprime to 256 and to 304 = 16 * 19; chosen with tools/gate_balance_model.py
#define IDN_TILE_SKEW 97

// the definition, in closed form (a division: not for the kernel's loop)
IDN_TILE_HD long tile_order_tile(long round, int c, int G) {
    return round * G + (long)(((long)c + round * IDN_TILE_SKEW) % G);
}

// per-round step of the rotation, IDN_TILE_SKEW mod G: computed once per launch, on the host
IDN_TILE_HD int tile_order_step(int G) { return IDN_TILE_SKEW % G; }

// The walk.  State: base = r * G and off = (c + r * kTileSkew) mod G, starting at (0, c); the current tile is base + off.
// Moves the state to round r + 1 and returns that round's tile.  step = tile_order_step(G) < G, so one subtraction wraps.
IDN_TILE_HD long tile_order_next(long* base, int* off, int G, int step) {
    int o = *off + step;
    o = o >= G ? o - G : o;
    *off = o;
    *base += G;
    return *base + o;
}
