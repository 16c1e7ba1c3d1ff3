// poly_alloc.hip -- note on/off for the poly voice bank with envelope-aware voice allocation, on the device,
// for gfx950 (MI355X).  The rule (include/synth_mi355x.h) is sequential: events in order, each
// note_on takes the free voice of lowest index, or else the voice of smallest key (gate, level, index).  The
// voices' envelope state lives in HBM, so the search runs here, in two kernels per launch of <= POLY_EV_CAP events:
//
// (1) poly_alloc_scan, one pass over inc/gate/stage/level (only for launches that hold a note_on).  Workgroup g
//     takes a contiguous run of voices and leaves, as of the batch start,
//       - the first POLY_LIST free voices of its run, in index order (wave ballots + per-wave counts), and
//       - the POLY_LIST smallest keys of its run's non-free voices, sorted: keys that beat the current 128th best
//         are compacted into an LDS buffer, and the buffer is bitonic-sorted into the best list when it fills.
//     key = gate << 63 | level << 31 | index  (index < 2^31): lexicographic (gate, level, index) in one u64.
// (2) poly_alloc_apply, one workgroup.  All its threads merge the per-workgroup lists (free: concatenation in
//     workgroup order; keys: a tree of "min against the reversed partner + bitonic merge" steps in LDS), then ONE
//     wave replays the events against the two global lists and a dirty set: the voices this launch has touched,
//     with their current inc/gate/stage/note.  A voice that nobody touched keeps its batch-start status and key,
//     so the best free voice is min(first untouched list entry, smallest free dirty voice), and the best steal
//     min(first untouched key, smallest dirty non-free key).  Each event touches at most two voices (a note_on of
//     a held note releases one and picks one), so with E <= 64 events fewer than 2E <= POLY_LIST voices are ever
//     touched before a pick: a full list never runs dry, and a list that is not full holds every such voice.
//     The dirty set and the note map are written back at the end.
//
// Controllers.  The op word is note | kind << 8.  Besides note_off / note_on, a note_off under a
// down pedal (OP_SUSTAIN) and "sustain every mapped note" (OP_SUSTAIN_ALL, CC 123 under the pedal) only set bits of
// sustained[128], which sits in LDS next to n2v.  The release-alls -- pedal up (OP_RELEASE_SUSTAINED) and CC 123 with
// the pedal up (OP_OFF_ALL) -- may touch up to 128 voices, which would break the 2-per-event bound above and the
// dirty set.  The host therefore gives each of them a launch of its own (no scan: nothing is picked).  There the
// dirty set is empty, note2voice is injective, and a release writes only gate and voice_note of its own voice, so
// the <= 128 releases are independent: wave 0 applies them in parallel, two notes per lane, straight to HBM.  All
// sound off (CC 120) is poly_sound_off below, a grid-stride kernel of its own, queued in stream order.
#include "smx_common.h"

namespace {

enum { ENV_IDLE = 0, ENV_R = 4 };
enum { OP_OFF = smx::POLY_OP_OFF, OP_ON = smx::POLY_OP_ON, OP_SUSTAIN = smx::POLY_OP_SUSTAIN,
       OP_SUSTAIN_ALL = smx::POLY_OP_SUSTAIN_ALL, OP_RELEASE_SUSTAINED = smx::POLY_OP_RELEASE_SUSTAINED,
       OP_OFF_ALL = smx::POLY_OP_OFF_ALL };
enum { POLY_LIST = 128, SCAN_NT = 512, SCAN_BUF = 1024, APPLY_NT = 1024 };
static_assert(POLY_LIST >= 2 * smx::POLY_EV_CAP, "the lists must outlast 2 touches per event");

constexpr uint64_t NO_KEY = ~0ull;
constexpr uint32_t NO_VOICE = 0xFFFFFFFFu;

__device__ inline uint64_t voice_key(uint32_t gate, uint32_t level, uint32_t v)
{
    return ((uint64_t)(gate != 0) << 63) | ((uint64_t)level << 31) | v;
}

__device__ inline bool voice_free(uint32_t inc, uint32_t gate, uint32_t stage)
{
    return inc == 0 || (gate == 0 && stage == ENV_IDLE);
}

// Ascending bitonic sort of s[0..N) by the NT threads of the workgroup (N = 2 * NT * k).
template <int N, int NT>
__device__ void bitonic_sort(uint64_t *s)
{
    for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < N / 2; t += NT) {
                const uint32_t i = (t / j) * 2 * j + (t % j), l = i + j;
                const bool up = (i & k) == 0;
                const uint64_t a = s[i], b = s[l];
                if ((a > b) == up) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
}

// Output of workgroup g: free_cnt[g], free_v[g][POLY_LIST], keys[g][POLY_LIST] (sorted, NO_KEY padded)
struct ScanOut {
    uint32_t *free_cnt, *free_v;
    uint64_t *keys;
};

__global__ __launch_bounds__(SCAN_NT)
void poly_alloc_scan(const uint32_t *__restrict__ inc, const uint32_t *__restrict__ gate,
                     const uint32_t *__restrict__ stage, const uint32_t *__restrict__ level,
                     uint32_t n, uint32_t tiles_per_wg, ScanOut out)
{
    __shared__ uint64_t buf[SCAN_BUF];           // [0, POLY_LIST): best so far; then candidates
    __shared__ uint32_t fl[POLY_LIST];
    __shared__ uint32_t wcnt[2][SCAN_NT / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (uint32_t i = tid; i < POLY_LIST; i += SCAN_NT) { buf[i] = NO_KEY; fl[i] = NO_VOICE; }
    uint64_t thresh = NO_KEY;                    // the current POLY_LIST-th best key (uniform)
    uint32_t nbuf = 0, fcnt = 0;                 // uniform copies
    __syncthreads();

    auto sort_in = [&]() {                       // buf[0, POLY_LIST + nbuf) -> best POLY_LIST in buf[0, POLY_LIST)
        for (uint32_t i = POLY_LIST + nbuf + tid; i < SCAN_BUF; i += SCAN_NT) buf[i] = NO_KEY;
        __syncthreads();
        bitonic_sort<SCAN_BUF, SCAN_NT>(buf);
        thresh = buf[POLY_LIST - 1];
        nbuf = 0;
    };

    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint64_t lt_mask = (1ull << lane) - 1;
    uint32_t vi = 0, vg = 0, vs = 0, vl = 0;
    auto load = [&](uint32_t t) {                // tile t of the bank (voices >= n are padding: skipped)
        const uint32_t v = t * SCAN_NT + tid;
        if (v < n) { vi = inc[v]; vg = gate[v]; vs = stage[v]; vl = level[v]; }
    };
    load(t0);
    for (uint32_t t = t0; t < t0 + tiles_per_wg && t * SCAN_NT < n; t++) {
        const uint32_t v = t * SCAN_NT + tid;
        const bool valid = v < n;
        const bool fr = valid && voice_free(vi, vg, vs);
        const uint64_t key = (valid && !fr) ? voice_key(vg, vl, v) : NO_KEY;
        if (t + 1 < t0 + tiles_per_wg) load(t + 1);          // the next tile's loads in flight meanwhile
        const bool c = key < thresh;
        const uint64_t mf = __ballot(fr), mc = __ballot(c);
        if (lane == 0) { wcnt[0][w] = __popcll(mf); wcnt[1][w] = __popcll(mc); }
        __syncthreads();
        uint32_t pf = 0, pc = 0, tf = 0, tc = 0;
        for (uint32_t k = 0; k < SCAN_NT / 64; k++) {
            const uint32_t a = wcnt[0][k], b = wcnt[1][k];
            if (k < w) { pf += a; pc += b; }
            tf += a; tc += b;
        }
        pf += __popcll(mf & lt_mask);
        pc += __popcll(mc & lt_mask);
        if (fr && fcnt + pf < POLY_LIST) fl[fcnt + pf] = v;
        fcnt = fcnt + tf < POLY_LIST ? fcnt + tf : POLY_LIST;
        if (tc) {
            if (POLY_LIST + nbuf + tc > SCAN_BUF) sort_in();   // room for a whole tile of candidates
            if (c) buf[POLY_LIST + nbuf + pc] = key;
            nbuf += tc;
        }
        __syncthreads();                                       // wcnt is rewritten by the next tile
    }
    if (nbuf) sort_in();
    const uint32_t g = blockIdx.x;
    for (uint32_t i = tid; i < POLY_LIST; i += SCAN_NT) {
        out.keys[(size_t)g * POLY_LIST + i] = buf[i];
        out.free_v[(size_t)g * POLY_LIST + i] = fl[i];
    }
    if (tid == 0) out.free_cnt[g] = fcnt;
}

// ---- the sequential replay: one wave ---------------------------------------------------------------------------
__device__ inline void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ inline uint32_t wmin32(uint32_t x)
{
    for (int o = 32; o; o >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)x, o); x = y < x ? y : x; }
    return x;
}
__device__ inline uint64_t wmin64(uint64_t x)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o);
        const uint64_t y = (uint64_t)hi << 32 | lo;
        x = y < x ? y : x;
    }
    return x;
}

struct ApplyArgs {
    uint32_t *inc, *gate, *stage;
    const uint32_t *level;
    int32_t *note2voice;             // [128], -1: none
    int32_t *voice_note;             // [n_pad], -1: none
    uint8_t *sustained;              // [128], 1: the note is held by the pedal
    const uint32_t *ops;             // n_ops pairs (note | kind << 8, inc of the note)
    uint32_t n_ops;
    uint32_t n_lists;                // workgroups of the scan (0: no scan ran -- the launch has no note_on)
    ScanOut lists;
};

__global__ __launch_bounds__(APPLY_NT)
void poly_alloc_apply(ApplyArgs A)
{
    // the scan's key lists, merged in place: LK[list][POLY_LIST]; list 0 ends up holding the global best
    extern __shared__ uint64_t LK[];
    __shared__ uint32_t FL[POLY_LIST], foff[APPLY_NT / 8];
    __shared__ uint32_t s_nfl;
    __shared__ uint8_t fdead[POLY_LIST], kdead[POLY_LIST];
    // dirty set
    __shared__ uint32_t Dv[POLY_LIST], Dinc[POLY_LIST], Dgate[POLY_LIST], Dstage[POLY_LIST], Dlevel[POLY_LIST];
    __shared__ int32_t Dnote[POLY_LIST];
    __shared__ int32_t n2v[128];
    __shared__ uint8_t sus[128];
    __shared__ uint32_t s_nd;
    const uint32_t tid = threadIdx.x;
    const uint32_t G = A.n_lists;
    uint32_t Gp = 1;
    while (Gp < G) Gp <<= 1;

    // (a) merge the lists (all threads)
    if (G) {
        for (uint32_t i = tid; i < Gp * POLY_LIST; i += APPLY_NT) LK[i] = i < G * POLY_LIST ? A.lists.keys[i] : NO_KEY;
        if (tid == 0) {                              // free lists: first POLY_LIST of the concatenation
            uint32_t acc = 0;
            for (uint32_t g = 0; g < G; g++) {
                foff[g] = acc;
                const uint32_t c = A.lists.free_cnt[g];
                acc = acc + c < POLY_LIST ? acc + c : POLY_LIST;
            }
            s_nfl = acc;
        }
        __syncthreads();
        for (uint32_t i = tid; i < G * POLY_LIST; i += APPLY_NT) {
            const uint32_t g = i / POLY_LIST, j = i % POLY_LIST;
            if (j < A.lists.free_cnt[g] && foff[g] + j < POLY_LIST) FL[foff[g] + j] = A.lists.free_v[i];
        }
        for (uint32_t s = 1; s < Gp; s <<= 1) {
            const uint32_t pairs = Gp / (2 * s);
            for (uint32_t i = tid; i < pairs * POLY_LIST; i += APPLY_NT) {     // a[j] = min(a[j], b[127 - j])
                uint64_t *a = LK + (size_t)(i / POLY_LIST) * 2 * s * POLY_LIST;
                const uint64_t *b = a + (size_t)s * POLY_LIST;
                const uint32_t j = i % POLY_LIST;
                const uint64_t y = b[POLY_LIST - 1 - j];
                if (y < a[j]) a[j] = y;
            }
            __syncthreads();
            for (uint32_t h = POLY_LIST / 2; h; h >>= 1) {                     // bitonic -> ascending
                for (uint32_t i = tid; i < pairs * POLY_LIST / 2; i += APPLY_NT) {
                    uint64_t *a = LK + (size_t)(i / (POLY_LIST / 2)) * 2 * s * POLY_LIST;
                    const uint32_t t = i % (POLY_LIST / 2), j = (t / h) * 2 * h + (t % h);
                    const uint64_t x = a[j], y = a[j + h];
                    if (x > y) { a[j] = y; a[j + h] = x; }
                }
                __syncthreads();
            }
        }
    } else {
        if (tid == 0) s_nfl = 0;
        for (uint32_t i = tid; i < POLY_LIST; i += APPLY_NT) LK[i] = NO_KEY;
    }
    for (uint32_t i = tid; i < POLY_LIST; i += APPLY_NT) { fdead[i] = 0; kdead[i] = 0; }
    for (uint32_t i = tid; i < 128; i += APPLY_NT) { n2v[i] = A.note2voice[i]; sus[i] = A.sustained[i]; }
    if (tid == 0) s_nd = 0;
    __syncthreads();
    if (tid >= 64) return;

    // a release-all, alone in its launch (the host guarantees it): independent releases of distinct voices
    const uint32_t kind0 = (A.ops[0] >> 8) & 7u;
    if (A.n_ops == 1 && (kind0 == OP_RELEASE_SUSTAINED || kind0 == OP_OFF_ALL)) {
        for (uint32_t m = tid; m < 128; m += 64) {
            const int32_t v = n2v[m];
            if (v >= 0 && (kind0 == OP_OFF_ALL || sus[m])) {
                A.gate[v] = 0;
                A.voice_note[v] = -1;
                n2v[m] = -1;
            }
            A.note2voice[m] = n2v[m];
            A.sustained[m] = 0;
        }
        return;
    }

    // (b) the events, in order, by wave 0.  Lane l looks after dirty entries / list positions l and l + 64.
    const uint32_t lane = tid;
    const uint32_t nfl = s_nfl;
    uint32_t fhead = 0, khead = 0;
    // the dirty index of voice v; a voice seen for the first time is read from HBM and struck from both lists
    auto touch = [&](uint32_t v) -> uint32_t {
        const uint32_t nd = s_nd;
        const bool hit0 = lane < nd && Dv[lane] == v, hit1 = lane + 64 < nd && Dv[lane + 64] == v;
        const uint64_t m0 = __ballot(hit0), m1 = __ballot(hit1);
        if (m0) return (uint32_t)__builtin_ctzll(m0);
        if (m1) return 64u + (uint32_t)__builtin_ctzll(m1);
        if (lane == 0) {
            Dv[nd] = v; Dinc[nd] = A.inc[v]; Dgate[nd] = A.gate[v]; Dstage[nd] = A.stage[v];
            Dlevel[nd] = A.level[v]; Dnote[nd] = A.voice_note[v];
            s_nd = nd + 1;
        }
        for (uint32_t i = lane; i < POLY_LIST; i += 64) {
            if (i < nfl && FL[i] == v) fdead[i] = 1;
            const uint64_t k = LK[i];
            if (k != NO_KEY && (uint32_t)(k & 0x7FFFFFFFu) == v) kdead[i] = 1;
        }
        wsync();
        return nd;
    };
    auto release = [&](int32_t note) {               // note_off of a mapped note
        const uint32_t v = (uint32_t)n2v[note];
        const uint32_t d = touch(v);
        if (lane == 0) { Dgate[d] = 0; Dnote[d] = -1; n2v[note] = -1; sus[note] = 0; }
        wsync();
    };
    auto pick = [&]() -> uint32_t {
        while (fhead < nfl && fdead[fhead]) fhead++;
        const uint32_t nd = s_nd;
        uint32_t dv = NO_VOICE;
        uint64_t dk = NO_KEY;
        for (uint32_t i = lane; i < nd; i += 64) {
            if (voice_free(Dinc[i], Dgate[i], Dstage[i])) dv = min(dv, Dv[i]);
            else dk = min(dk, voice_key(Dgate[i], Dlevel[i], Dv[i]));
        }
        dv = wmin32(dv);
        const uint32_t fv = fhead < nfl ? FL[fhead] : NO_VOICE;
        if (dv != NO_VOICE || fv != NO_VOICE) return min(dv, fv);
        dk = wmin64(dk);
        while (khead < POLY_LIST && kdead[khead]) khead++;
        const uint64_t kk = khead < POLY_LIST ? LK[khead] : NO_KEY;
        const uint64_t best = min(dk, kk);
        return best == NO_KEY ? NO_VOICE : (uint32_t)(best & 0x7FFFFFFFu);
    };

    for (uint32_t e = 0; e < A.n_ops; e++) {
        const uint32_t op = A.ops[2 * e], ninc = A.ops[2 * e + 1];
        const int32_t note = (int32_t)(op & 127u);
        const uint32_t kind = (op >> 8) & 7u;
        if (kind == OP_SUSTAIN || kind == OP_SUSTAIN_ALL) {          // the pedal keeps the voice: gate and maps stay
            for (uint32_t m = lane; m < 128; m += 64)
                if ((kind == OP_SUSTAIN_ALL || m == (uint32_t)note) && n2v[m] >= 0) sus[m] = 1;
            wsync();
            continue;
        }
        if (n2v[note] >= 0) release(note);          // note_off, or a note_on of a held (or sustained) note
        if (kind != OP_ON) continue;
        const uint32_t v = pick();
        if (v == NO_VOICE) continue;                 // unreachable for n >= 1 (every voice is free or has a key)
        const uint32_t d = touch(v);
        if (lane == 0) {
            if (Dnote[d] >= 0) { n2v[Dnote[d]] = -1; sus[Dnote[d]] = 0; }
            if (Dgate[d]) Dstage[d] = ENV_R;         // a held voice is stolen: the block start re-attacks it
            Dinc[d] = ninc; Dgate[d] = 1; Dnote[d] = note; n2v[note] = (int32_t)v;
        }
        wsync();
    }

    // (c) write back
    const uint32_t nd = s_nd;
    for (uint32_t i = lane; i < nd; i += 64) {
        const uint32_t v = Dv[i];
        A.inc[v] = Dinc[i]; A.gate[v] = Dgate[i]; A.stage[v] = Dstage[i]; A.voice_note[v] = Dnote[i];
    }
    for (uint32_t i = lane; i < 128; i += 64) { A.note2voice[i] = n2v[i]; A.sustained[i] = sus[i]; }
}

// All sound off (CC 120): every voice idle, silent and free; both maps and the sustained bits cleared.  inc, phase,
// y and the patch are not touched.  16 B written per voice.
__global__ __launch_bounds__(256)
void poly_sound_off(uint32_t *__restrict__ gate, uint32_t *__restrict__ stage, uint32_t *__restrict__ level,
                    int32_t *__restrict__ voice_note, int32_t *__restrict__ note2voice, uint8_t *__restrict__ sustained,
                    uint32_t n_pad)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 128) { note2voice[threadIdx.x] = -1; sustained[threadIdx.x] = 0; }
    for (uint32_t v = t; v < n_pad; v += gridDim.x * 256) {
        gate[v] = 0; stage[v] = ENV_IDLE; level[v] = 0; voice_note[v] = -1;
    }
}

}  // namespace

namespace smx {

uint32_t poly_alloc_lists(uint32_t n)
{
    const uint32_t tiles = (n + SCAN_NT - 1) / SCAN_NT;
    return tiles < POLY_ALLOC_MAX_WG ? tiles : POLY_ALLOC_MAX_WG;
}

size_t poly_alloc_scratch_bytes(uint32_t n)
{
    const size_t g = poly_alloc_lists(n);
    return g * POLY_LIST * 8 + g * POLY_LIST * 4 + g * 4;
}

int launch_poly_alloc(const PolyArrays &p, int32_t *d_note2voice, int32_t *d_voice_note, uint8_t *d_sustained,
                      const uint32_t *d_ops, uint32_t n_ops, bool any_on, uint32_t n, void *d_scratch,
                      hipStream_t stream)
{
    if (n_ops == 0 || n_ops > POLY_EV_CAP || n == 0 || n >= 0x80000000u) {
        set_error("launch_poly_alloc: n_ops=%u n=%u", n_ops, n);
        return SMX_E_ARG;
    }
    const uint32_t G = poly_alloc_lists(n);
    ScanOut lists;
    lists.keys = (uint64_t *)d_scratch;
    lists.free_v = (uint32_t *)(lists.keys + (size_t)G * POLY_LIST);
    lists.free_cnt = lists.free_v + (size_t)G * POLY_LIST;
    if (any_on) {
        const uint32_t tiles = (n + SCAN_NT - 1) / SCAN_NT;
        const uint32_t tpw = (tiles + G - 1) / G;
        const uint32_t gx = (tiles + tpw - 1) / tpw;             // <= G; workgroups [gx, G) would have no voices
        hipLaunchKernelGGL(poly_alloc_scan, dim3(gx), dim3(SCAN_NT), 0, stream, p.inc, p.gate, p.stage, p.level,
                           n, tpw, lists);
        SMX_HIP(hipGetLastError());
        ApplyArgs a{p.inc, p.gate, p.stage, p.level, d_note2voice, d_voice_note, d_sustained, d_ops, n_ops, gx, lists};
        uint32_t gp = 1;
        while (gp < gx) gp <<= 1;
        static const bool lds_ok = hipFuncSetAttribute((const void *)poly_alloc_apply,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       POLY_ALLOC_MAX_WG * POLY_LIST * 8) == hipSuccess;
        if (!lds_ok) { set_error("launch_poly_alloc: cannot raise the LDS limit of poly_alloc_apply"); return SMX_E_NOGPU; }
        hipLaunchKernelGGL(poly_alloc_apply, dim3(1), dim3(APPLY_NT), (size_t)gp * POLY_LIST * 8, stream, a);
    } else {
        ApplyArgs a{p.inc, p.gate, p.stage, p.level, d_note2voice, d_voice_note, d_sustained, d_ops, n_ops, 0, lists};
        hipLaunchKernelGGL(poly_alloc_apply, dim3(1), dim3(APPLY_NT), (size_t)POLY_LIST * 8, stream, a);
    }
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_poly_sound_off(const PolyArrays &p, int32_t *d_note2voice, int32_t *d_voice_note, uint8_t *d_sustained,
                          uint32_t n_pad, hipStream_t stream)
{
    if (n_pad == 0 || (n_pad & 1023)) { set_error("launch_poly_sound_off: n_pad=%u", n_pad); return SMX_E_ARG; }
    const uint32_t blocks = n_pad / 256;
    const uint32_t gx = blocks < 2048u ? blocks : 2048u;     // 8 workgroups per CU, grid-stride above that
    hipLaunchKernelGGL(poly_sound_off, dim3(gx), dim3(256), 0, stream, p.gate, p.stage, p.level, d_voice_note,
                       d_note2voice, d_sustained, n_pad);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
