// Index arithmetic of orb_fast_kernel's LDS carve, shared by the kernel, its launch (corb_launch_orb_pipeline), the create-time geometry
// (corb_orb.cpp) and a host check (tests/test_fast_tile_index.py compiles this header alone with the host compiler).
//
// The cell tile holds one 16-bit SLOT per pixel, TP slots per row: the low byte is the pixel, the high byte its FAST score (0 until phase 2 scores
// the pixel, 0 = not a corner).  An aligned dword of a tile row is a pixel pair [b(k),s(k) | b(k+1),s(k+1)] with k even: with the score bytes
// masked off (one v_and_b32, or the zero selectors of a v_perm_b32) it is the operand format of the packed 16-bit min/max chain.  Tile column k <-> image x = iniX - 1 + k: column 0 is
// padding, columns 1..3 the left halo, the interior (scored pixels) starts at column 4 = dword 2 = byte 8 of the row, and a row is a multiple of
// 8 bytes, so a 4-pixel group g (columns 4g+4 .. 4g+7) is the two dwords of ONE aligned 8-byte word.
//
// Padding rule: a row has TP >= 4 * ceil(wCell / 4) + 8 slots and EVERY slot of the rows 0 .. ch-1 is written from the image (byte-valued), so
// that the widest window (columns 4g .. 4g+11 of the last group) stays inside its own row: no window dword ever leaves initialised slots, whatever
// the cell's width, and a half past the cell's last pixel only ever holds a byte once masked (it is masked out of the result, and being <= 0xff it
// cannot carry into the valid half of a 32-bit add).  Scores are only ever written to interior pixels, so halo and padding slots keep a zero high byte.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FAST_TILE_HD __host__ __device__ inline
#else
#define FAST_TILE_HD inline
#endif

#define FAST_LIST_CAP 512          // entries of the pixel-pair list (uint16_t, static LDS): four full sweeps
#define FAST_LIST_SWEEP 128        // room one sweep of the wave's patch may need: 64 lanes x 2 pairs

// tile pitch in slots that a level with cells of wCell interior columns needs: pad + halo (4) + 4-px groups + the right window columns
FAST_TILE_HD int fast_tile_min_pitch(int wCell) { return 4 * ((wCell + 3) / 4) + 8; }
// the instantiated pitch (orb_fast_kernel<TP>) that serves a required pitch
FAST_TILE_HD int fast_tile_pitch_class(int tp) { return tp <= 40 ? 40 : tp <= 48 ? 48 : 80; }
FAST_TILE_HD int fast_tile_row_dwords(int TP) { return TP / 2; }                    // a row of TP 16-bit slots
FAST_TILE_HD int fast_tile_groups(int cw) { return (cw - 6 + 3) >> 2; }              // 4-pixel groups per interior row
// dword of a row that holds the pair `pair` (0, 1) of group g: interior column 4g + 2 * pair
FAST_TILE_HD int fast_tile_pair_dword(int g, int pair) { return 2 * g + 2 + pair; }

// Phase 1 (compass test of a group): rows y - 3 and y + 3 give the 8-byte word of the group itself, row y the three 8-byte words around it
// (dwords 2g .. 2g+5: the two centres, and the dx = -3 / +3 pairs as one byte permute of two adjacent dwords each).
FAST_TILE_HD int fast_tile_compass_first(int g, int dy) { return dy == 0 ? 2 * g : 2 * g + 2; }
FAST_TILE_HD int fast_tile_compass_count(int dy) { return dy == 0 ? 6 : 2; }

// Phase 2 (ring of a listed pair at dword q of row y): the dwords of row y + dy, relative to q.  dx = 0, +-2 are dwords as they stand, dx = +-1, +-3
// take the high slot of the lower and the low slot of the upper of two adjacent dwords.
//   |dy| = 3: dx = -1, 0, 1   -> q-1, q, q+1         |dy| = 2: dx = -2, 2 -> q-1, q+1
//   |dy| = 1: dx = -3, 3      -> q-2, q-1, q+1, q+2   dy  = 0: dx = -3, centre, 3 -> q-2 .. q+2
FAST_TILE_HD int fast_tile_ring_reach(int dy) { const int a = dy < 0 ? -dy : dy; return a >= 2 ? 1 : 2; }          // reads lie in q - reach .. q + reach
FAST_TILE_HD bool fast_tile_ring_reads(int dy, int k)                                                                // is dword q + k of row y + dy read?
{
    const int a = dy < 0 ? -dy : dy, b = k < 0 ? -k : k;
    return a == 3 ? b <= 1 : a == 2 ? b == 1 : a == 1 ? (b == 1 || b == 2) : b <= 2;
}

// Phase 3 (strict 8-neighbour maximum of a pair's two scores): dwords q-1, q, q+1 of the rows y-1, y, y+1 -- inside phase 2's reach.
FAST_TILE_HD int fast_tile_nms_reach() { return 1; }

// ---- the carve: [tile | row masks] in dynamic LDS, the pair list in static LDS ----
FAST_TILE_HD unsigned fast_tile_bytes(int TP, int th) { return 2u * (unsigned)TP * (unsigned)th; }
FAST_TILE_HD unsigned fast_rowmask_bytes(int th) { return 8u * (unsigned)(th - 6); }                               // two dwords per interior row
FAST_TILE_HD unsigned fast_dynamic_lds_bytes(int TP, int th) { return fast_tile_bytes(TP, th) + fast_rowmask_bytes(th); }
FAST_TILE_HD unsigned fast_cell_lds_bytes(int TP, int th) { return fast_dynamic_lds_bytes(TP, th) + 2u * FAST_LIST_CAP; }
