// stage_map.hpp — index maps of the un-pooling staging loops: which pooled element an item of a block loads and which slots of the
// block's LDS halo image it fills.  Shared by the kernels and by the host entry clhip_internal_stage_map (tests/test_stage_map_cpu.py checks
// the maps there, without a GPU, against the per-pixel rule they replace).
//
// bf16-split backward-data behind a 2x2 pool (bsconv.hip, bs_conv_body<G, MODE, UNPOOL = true>).  The halo image of a chunk holds,
// per (halo pixel, k half), 8 channels of max_pool2d's backward: v = code == position ? pooled gradient : 0.  Staged per halo pixel
// every pooled value and code byte was fetched by the up to four pixels of its window — four items, 8 + 8 loads each.  Here an item is
// (image, halo row, WINDOW column, k half): it loads the 8 pooled values and 8 codes once and writes the window's two pixels of that
// row.  Per block and chunk a pooled value is loaded twice (once per halo row of its window) instead of four times, and every
// geometry stages in ONE round of 256 items where it took two: half the load instructions, half the staging registers, the same
// selects, splits and LDS writes.  (Whole 2x2 windows as items — each value loaded once — would leave 144 items for 256 threads on
// the 32 x 4 tile with four splits each: twice the VALU instructions per wave, which is what the matrix stream cannot hide.)
// A window cut by the left / right edge of the halo tile has ONE pixel inside: the item writes that pixel twice (same slot, same
// bits) so that no LDS write sits under a branch.  For the same reason the spare threads of the round (256 - ITEMS) stage too, but
// nothing real: their loads are out of range (no memory traffic, zeros) and their writes go to the padding slots behind the halo
// pixels of an LDS row (pitch P > row length), which no operand read touches.
#pragma once

struct BsStageItem {
    int ni, h, hy;          // image of the block, k half, halo row
    int hx[2];              // halo columns of the two pixels written (equal where the window is cut by the halo edge)
    int spare;              // >= 0: a spare thread of the round (ni = h = hy = hx = 0), its number
};

// G: a BsGeo of bsconv.hip
template <class G>
struct BsUnpoolMap {
    static constexpr int WO = G::HP & 1;                               // an odd halo starts on the right half of a window (tiles start on even columns)
    static constexpr int NWC = (G::HW_ + WO + 1) / 2;                  // window columns of one image's halo row
    static constexpr int NWIN = G::NI * G::HR * NWC;
    static constexpr int ITEMS = 2 * NWIN;                             // (window of a halo row, k half)
    static constexpr int ROUNDS = (ITEMS + 255) / 256;
    static_assert(G::RW % 2 == 0 && G::HW_ % 2 == 0, "tiles start and end on window boundaries");
    static constexpr int PAD = G::P - G::IPR * G::HW_;                 // padding slots of an LDS row (every row but the last has them)
    static_assert(PAD >= 1 && G::ROWS >= 2, "somewhere for the spare threads to write");

    // item `it` of [0, ROUNDS * 256); the ones past ITEMS are the spare threads
    __host__ __device__ static BsStageItem item(int it) {
        BsStageItem s;
        s.spare = it - ITEMS;
        if (it >= ITEMS) it = 0;
        s.h = it >= NWIN ? 1 : 0;
        const int p = it - s.h * NWIN;
        s.ni = p / (G::HR * NWC);
        const int rem = p - s.ni * (G::HR * NWC);
        s.hy = rem / NWC;
        const int wc = rem - s.hy * NWC, a = 2 * wc - WO;
        s.hx[0] = a < 0 ? 0 : a;
        s.hx[1] = a + 1 > G::HW_ - 1 ? G::HW_ - 1 : a + 1;
        return s;
    }
    // LDS slot (16 bytes) of (k half, image, halo row, halo column) inside the plane pair of one bf16 piece
    __host__ __device__ static int slot(int h, int ni, int hy, int hx) {
        return h * G::PLANE_SLOTS + ((ni / G::IPR) * G::HR + hy) * G::P + (ni % G::IPR) * G::HW_ + hx;
    }
    // ... that pixel p of item s writes
    __host__ __device__ static int slot(const BsStageItem& s, int p) {
        if (s.spare >= 0) return (s.spare / PAD) % (G::ROWS - 1) * G::P + G::IPR * G::HW_ + s.spare % PAD;
        return slot(s.h, s.ni, s.hy, s.hx[p]);
    }
};

// What item s of the tile at (image n0, row y0, column x0) loads: the offset, in elements from image n0 of the pooled tensor
// [N][Cin][H / 2][W / 2], of channel 8 h of chunk 0 — or -1: the window lies outside the image (or the image past the batch), or the
// item is a spare thread's, and it stages zeros.  pos[p]: the window position (2 * row parity + column parity) whose arg-max code keeps the value in pixel p.
// Both pixels lie in one window (H, W and x0 are even), so one test serves both.
template <class G>
__host__ __device__ inline int bs_unpool_source(const BsStageItem& s, int n0, int y0, int x0, int N, int Cin, int H, int W, int (&pos)[2]) {
    const int gy = y0 + s.hy - G::HP, gx = x0 + s.hx[0] - G::HP;
    pos[0] = ((gy & 1) << 1) | (gx & 1);
    pos[1] = ((gy & 1) << 1) | ((x0 + s.hx[1] - G::HP) & 1);
    const bool ok = s.spare < 0 && n0 + s.ni < N && gy >= 0 && gy < H && gx >= 0 && gx < W;
    return ok ? (s.ni * Cin + 8 * s.h) * ((H >> 1) * (W >> 1)) + (gy >> 1) * (W >> 1) + (gx >> 1) : -1;
}

// pixel block pb of a launch -> first image, first row, first column of its tile
template <class G>
__host__ __device__ inline void bs_tile_origin(int pb, int tiles_x, int tiles_y, int& n0, int& y0, int& x0) {
    const int tx = pb % tiles_x, ty = (pb / tiles_x) % tiles_y, grp = pb / (tiles_x * tiles_y);
    n0 = grp * G::NI; y0 = ty * G::RH; x0 = tx * G::RW;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Winograd backward-data behind a 2x2 pool (wino.hip, wino_conv16g_body<TC, TR, EROWS, 1, UNPOOL = true>).  A chunk buffer holds the
// halo planes of 4 channels: float [channel][entity][PRE = 2 EROWS + 2 rows][PW = 2 TC + 2 columns], halo row / column 0 = image row /
// column (first of the entity) - 1 — odd, so the halo cuts the windows of its first and last row and column in half.  Staged per
// halo element (one 4-byte load, one code byte, one select, one LDS write each) a pooled value was fetched up to four times.  Here an
// item is a pooled WINDOW of (channel, entity): one value + one code loaded, four selects, four LDS writes; (EROWS + 2) x (TC + 2)
// windows per plane.  A pixel of a cut window that falls outside the halo is written onto the nearest pixel inside instead — a pixel
// of the same window, with that pixel's own position, so the slot gets the same bits twice and no write sits under a branch.
struct W16gStageItem {
    int cl, ent, wr, wc;    // channel of the chunk, entity of the block, window row / column inside the entity's halo
    int idx[4], pos[4];     // per pixel 2 r + c: float index inside the chunk buffer, window position kept there
};

template <int TC, int TR, int EROWS>
struct W16gUnpoolMap {
    static constexpr int CQ = 4, NE = 2 * TR / EROWS, PW = 2 * TC + 2, PRE = 2 * EROWS + 2, PLANE = NE * PRE * PW;
    static constexpr int NWR = EROWS + 2, NWC = TC + 2, ITEMS = CQ * NE * NWR * NWC, ROUNDS = (ITEMS + 255) / 256;

    __host__ __device__ static W16gStageItem item(int e) {
        W16gStageItem s;
        s.cl = e / (NE * NWR * NWC);
        int rem = e - s.cl * (NE * NWR * NWC);
        s.ent = rem / (NWR * NWC);
        rem -= s.ent * (NWR * NWC);
        s.wr = rem / NWC;
        s.wc = rem - s.wr * NWC;
        for (int p = 0; p < 4; ++p) {
            int row = 2 * s.wr - 1 + (p >> 1), col = 2 * s.wc - 1 + (p & 1);
            row = row < 0 ? 0 : row > PRE - 1 ? PRE - 1 : row;
            col = col < 0 ? 0 : col > PW - 1 ? PW - 1 : col;
            s.idx[p] = s.cl * PLANE + (s.ent * PRE + row) * PW + col;
            s.pos[p] = (((row + 1) & 1) << 1) | ((col + 1) & 1);       // (halo row 0 is an odd image row, halo column 0 an odd image column)
        }
        return s;
    }
    // the pooled element item s loads: offset in elements from image nb0 = v0 / tiles_h of the pooled tensor [N][Cin][H / 2][W / 2]
    // (channel cl of chunk 0), or -1 outside the image / past the batch.  v0: first entity of the block (entities count (image, row
    // group of 2 EROWS image rows), tiles_h groups per image); w0: first image column of the block (even).
    __host__ __device__ static int source(const W16gStageItem& s, int v0, int w0, int tiles_h, int N, int Cin, int H, int W) {
        const int Hi = H >> 1, Wi = W >> 1, v = v0 + s.ent, nn = v / tiles_h, g = v - nn * tiles_h;
        const int ph = g * EROWS + s.wr - 1, pw = (w0 >> 1) + s.wc - 1;
        const bool ok = nn < N && ph >= 0 && ph < Hi && pw >= 0 && pw < Wi;
        return ok ? ((nn - v0 / tiles_h) * Cin + s.cl) * (Hi * Wi) + ph * Wi + pw : -1;
    }
};

// ------------------------------------------------------------------------------------------------------------------------------
// Plain (not un-pooling) staging of the one-image 8 x 8 Winograd kernel (wino.hip, wino_conv16_body<MODE, false, KT2>: forward of 8 x 8
// layers, backward-data without codes).  A chunk buffer holds the halo planes of 8 channels of the block's NIMG = KT2 whole images:
// float [channel][image][10 rows][10 columns].  On whole 8 x 8 images the halo ring is constant zero and the interior is 16 float4s per
// plane, but the buffer was staged one scalar per halo element: 7 loads + 7 LDS writes per thread and chunk (KT2 = 2; 4 + 4 for KT2 = 1),
// zeros included.  Here the ring of both chunk buffers is written once, in the prologue (nothing writes it afterwards), and an item is
// one float4 of an image row — a 16-byte load, four floats to LDS (two-dword writes: an interior row starts on an odd float): one item
// per thread and chunk (KT2 = 2: 256 items; KT2 = 1: 128, the upper two waves stage nothing).
template <int KT2>
struct W16PlainMap {
    static constexpr int NIMG = KT2, CK = 8, PW = 10, PR = 10, PLANE = NIMG * PR * PW;
    static constexpr int ITEMS = CK * NIMG * 16;                       // float4s of the interior
    static constexpr int RING = CK * NIMG * 36;                        // ring elements of one chunk buffer
    static_assert(ITEMS <= 256, "one item per thread");
    // item f: the float4's offset in elements from image n0's chunk (channel cl, image nb, row, half row) and its first LDS float
    __host__ __device__ static void item(int f, int Cin, int& nb, int& src, int& idx) {
        const int cl = f / (NIMG * 16), rem = f - cl * (NIMG * 16);
        nb = rem >> 4;
        const int row = (rem & 15) >> 1, half = rem & 1;
        src = (nb * Cin + cl) * 64 + row * 8 + half * 4;
        idx = cl * PLANE + (nb * PR + row + 1) * PW + 1 + half * 4;
    }
    // ring element r of [0, RING): its LDS float
    __host__ __device__ static int ring(int r) {
        const int pl = r / 36, k = r - pl * 36;                        // plane = (channel, image)
        const int row = k < 10 ? 0 : k < 20 ? 9 : 1 + ((k - 20) >> 1), col = k < 10 ? k : k < 20 ? k - 10 : ((k - 20) & 1) * 9;
        return pl * (PR * PW) + row * PW + col;
    }
};

/* Test hook, not part of the library's API (include/clhip.h does not declare it; tests bind it by name).
 * Staging map of the un-pooling backward-data kernels: a HOST function over HOST arrays, nothing is launched.  With idx
 * given, a block of clhip_conv3x3_bs_bwd_data rebuilds max_pool2d's backward while it stages its input tile in LDS: a staging item
 * loads 8 channels of ONE pooled element + their arg-max codes and writes the two pixels of that window's row (csrc/stage_map.hpp,
 * which the kernel and this entry share).  kernel: 0 = the bf16-split body; geo: its block geometry, 0 = 32 x 4 pixels, 1 = 32 x 2,
 * 2 = 16 x 8, 3 = two 8 x 8 images.  N, Cin, H, W as the kernel sees them (Cin = K of the layer, H x W the un-pooled map, even).
 * block < 0: returns the number of pixel blocks of the launch.  Otherwise write i of pixel block `block` (chunk 0; all of its
 * threads, the spare ones that repeat an item included) is: src[i] = element of the pooled tensor [N][Cin][H/2][W/2] whose channel
 * and the 7 behind it are loaded, or -1 (outside the image: zeros are staged); pos[i] = the window position the code is compared
 * with; slot[i] = 16-byte slot of the halo image [k half][row][pitch].  Returns the number of writes (the arrays take the first
 * `cap`).  kernel 1 = the 16-tile Winograd body (clhip_conv3x3_wino_bwd_data / _wino_bwd with idx), geo 0 = <8, 2, 4> (even maps
 * 16 or more wide), 1 = <4, 4, 4> (8 x 8 maps): an item is a whole pooled window of one channel, four writes each; src[i] = the
 * pooled element, slot[i] = float index inside the chunk buffer [4 channels][entity][halo row][halo column].
 * kernel 2 = the plain staging of the one-image 8 x 8 Winograd body (clhip_conv3x3_wino_fwd / _wino_bwd_data without idx on 8 x 8 maps),
 * geo = KT2 - 1 (0: one image per block, 1: two), H = W = 8, block = image group: an item is a float4 of an image row, four writes each
 * (src[i] = the element of the input tensor [N][Cin][8][8] that lands in the slot, pos[i] = -1), followed by the zero ring written in
 * the prologue (src = -1); slot[i] = float index inside the chunk buffer [8 channels][image][10][10].
 * CLHIP_ENOTSUP: unknown kernel / geo; CLHIP_EINVAL: a shape the kernel does not take, block past the launch. */
extern "C" __attribute__((visibility("default"))) int clhip_internal_stage_map(int kernel, int geo, int N, int Cin, int H, int W, int block, int* src, int* pos, int* slot, int cap);

// its kernels 1 and 2 (wino.hip)
int clhip_internal_wino_stage_map(int kernel, int geo, int N, int Cin, int H, int W, int block, int* src, int* pos, int* slot, int cap);
