// abi_poly.cpp -- part of the C-ABI of libsynth_mi355x.so (include/synth_mi355x.h): poly voice bank
// Host side of the drop-in boundary.  No CPU compute fallback exists: every compute entry
// point needs a HIP device and fails with SMX_E_NOGPU otherwise.
#include "abi_internal.h"
#include <cmath>
// ---------------------------------------------------------------------------
// poly voice bank (build-defined extension; BASELINE config 4)
// ---------------------------------------------------------------------------
struct smx_poly {
    uint32_t n = 0, n_pad = 0;
    int device = 0;
    smx::PolyArrays d{};               // device arrays
    int32_t *d_bus2 = nullptr;         // two buses of int32[2*64], used alternately (the fold of block k is done by launch k+1)
    int32_t *d_bus = nullptr;          // the bus of the last block
    uint32_t bus_k = 0;
    int32_t *d_slots = nullptr;        // bus copies the workgroups add into (poly_bank.hip), kept zero
    smx::PolyPending pend;             // the fold the last launch left to its successor
    int32_t *h_bus = nullptr;          // pinned
    hipStream_t stream = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    // note events (poly_alloc.hip): the maps live on the device, -1 = none
    int32_t *d_note2voice = nullptr;   // [128]
    int32_t *d_voice_note = nullptr;   // [n_pad]
    void *d_alloc = nullptr;           // the scan's per-workgroup lists
    uint8_t *d_sustained = nullptr;    // [128], 1: the note is held by the pedal
    // controllers: the pedal and the bend are functions of the event stream alone, so the host
    // tracks them; only the sustained bits live on the device
    bool controllers = false;
    bool pedal = false;
    int bend14 = 8192, bend_range = 2;
    uint32_t bend_mul = 65536u;        // passed to every render launch
    // a batch's parsed events (note | kind << 8, increment), staged in pinned memory: two slots, so the host fills
    // one while the copy of the other may still be in flight
    uint32_t *h_ops[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    bool ev_stage_busy[2] = {false, false};
    size_t ops_cap = 0;                // events per slot
    uint32_t *d_ops = nullptr;
    int ev_k = 0;
};

static void poly_slots(smx::PolyArrays &d, void **slots[12])
{
    slots[0] = (void **)&d.inc;   slots[1] = (void **)&d.phase; slots[2] = (void **)&d.y;
    slots[3] = (void **)&d.a;     slots[4] = (void **)&d.level; slots[5] = (void **)&d.stage;
    slots[6] = (void **)&d.gate;  slots[7] = (void **)&d.ar;    slots[8] = (void **)&d.dr;
    slots[9] = (void **)&d.sl;    slots[10] = (void **)&d.rr;   slots[11] = (void **)&d.pan;
}

extern "C" smx_poly *smx_poly_create(uint32_t n_voices, int device)
{
    if (n_voices == 0 || n_voices > 0xFFFFF000u) { set_error("smx_poly_create: n_voices=%u (1..2^32-4096)", n_voices); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("smx_poly_create: no HIP device (this library has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) { set_error("smx_poly_create: device %d of %d", device, ndev); return nullptr; }
    smx_poly *p = new smx_poly();
    p->n = n_voices;
    p->n_pad = smx::round_up(n_voices, 1024);
    p->device = device;
    const size_t bytes = (size_t)p->n_pad * 4;
    void **slots[12];
    poly_slots(p->d, slots);
    bool ok = hipSetDevice(device) == hipSuccess &&
              hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&p->ev_t0) == hipSuccess && hipEventCreate(&p->ev_t1) == hipSuccess &&
              hipMalloc((void **)&p->d_bus2, 2 * smx::poly_bus_bytes()) == hipSuccess &&
              hipMemsetAsync(p->d_bus2, 0, 2 * smx::poly_bus_bytes(), p->stream) == hipSuccess &&
              hipMalloc((void **)&p->d_slots, smx::poly_scratch_bytes()) == hipSuccess &&
              hipMemsetAsync(p->d_slots, 0, smx::poly_scratch_bytes(), p->stream) == hipSuccess &&
              hipHostMalloc((void **)&p->h_bus, 128 * 4, hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void **)&p->d_note2voice, 128 * 4) == hipSuccess &&
              hipMalloc((void **)&p->d_voice_note, bytes) == hipSuccess &&
              hipMemsetAsync(p->d_note2voice, 0xFF, 128 * 4, p->stream) == hipSuccess &&
              hipMemsetAsync(p->d_voice_note, 0xFF, bytes, p->stream) == hipSuccess &&
              hipMalloc(&p->d_alloc, smx::poly_alloc_scratch_bytes(n_voices)) == hipSuccess &&
              hipMalloc((void **)&p->d_sustained, 128) == hipSuccess &&
              hipMemsetAsync(p->d_sustained, 0, 128, p->stream) == hipSuccess;
    for (int i = 0; ok && i < 12; i++)
        ok = hipMalloc(slots[i], bytes) == hipSuccess &&
             hipMemsetAsync(*slots[i], 0, bytes, p->stream) == hipSuccess;   // inc 0: all voices off
    ok = ok && hipStreamSynchronize(p->stream) == hipSuccess;
    if (!ok) {
        set_error("smx_poly_create: HIP allocation failed: %s", hipGetErrorString(hipGetLastError()));
        smx_poly_destroy(p);
        return nullptr;
    }
    return p;
}

extern "C" void smx_poly_destroy(smx_poly *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    void **slots[12];
    poly_slots(p->d, slots);
    for (int i = 0; i < 12; i++)
        if (*slots[i]) (void)hipFree(*slots[i]);
    if (p->d_bus2) (void)hipFree(p->d_bus2);
    if (p->d_slots) (void)hipFree(p->d_slots);
    if (p->h_bus) (void)hipHostFree(p->h_bus);
    if (p->d_note2voice) (void)hipFree(p->d_note2voice);
    if (p->d_voice_note) (void)hipFree(p->d_voice_note);
    if (p->d_alloc) (void)hipFree(p->d_alloc);
    if (p->d_sustained) (void)hipFree(p->d_sustained);
    if (p->d_ops) (void)hipFree(p->d_ops);
    for (int i = 0; i < 2; i++) {
        if (p->h_ops[i]) (void)hipHostFree(p->h_ops[i]);
        if (p->ev_stage[i]) (void)hipEventDestroy(p->ev_stage[i]);
    }
    if (p->ev_t0) (void)hipEventDestroy(p->ev_t0);
    if (p->ev_t1) (void)hipEventDestroy(p->ev_t1);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

static int poly_copy(smx_poly *p, const struct smx_poly_arrays *a, bool to_device)
{
    if (!p || !a) return SMX_E_ARG;
    SMX_HIP(hipSetDevice(p->device));
    SMX_HIP(hipStreamSynchronize(p->stream));
    void **slots[12];
    poly_slots(p->d, slots);
    void *host[12] = {a->inc, a->phase, a->y, a->a, a->level, a->stage,
                      a->gate, a->ar, a->dr, a->sl, a->rr, a->pan};
    for (int i = 0; i < 12; i++) {
        if (!host[i]) continue;
        if (to_device) SMX_HIP(hipMemcpy(*slots[i], host[i], (size_t)p->n * 4, hipMemcpyHostToDevice));
        else           SMX_HIP(hipMemcpy(host[i], *slots[i], (size_t)p->n * 4, hipMemcpyDeviceToHost));
    }
    if (to_device && (a->inc || a->gate)) {          // new increments or gates: no voice holds a note any more
        SMX_HIP(hipMemsetAsync(p->d_note2voice, 0xFF, 128 * 4, p->stream));
        SMX_HIP(hipMemsetAsync(p->d_sustained, 0, 128, p->stream));
        SMX_HIP(hipMemsetAsync(p->d_voice_note, 0xFF, (size_t)p->n_pad * 4, p->stream));
        SMX_HIP(hipStreamSynchronize(p->stream));
    }
    return SMX_OK;
}

extern "C" int smx_poly_load(smx_poly *p, const struct smx_poly_arrays *a) { return poly_copy(p, a, true); }
extern "C" int smx_poly_read(smx_poly *p, const struct smx_poly_arrays *a) { return poly_copy(p, a, false); }

extern "C" int smx_poly_run_async(smx_poly *p, int n)
{
    if (!p || n <= 0 || n > 64) { set_error("smx_poly_run_async: n=%d (1..64)", n); return SMX_E_ARG; }
    SMX_HIP(hipSetDevice(p->device));
    static const bool no_defer = getenv("SMX_POLY_NO_DEFER") != nullptr;      // A/B switch: every launch folds its own copies
    p->d_bus = p->d_bus2 + (size_t)(p->bus_k++ & 1u) * (smx::poly_bus_bytes() / 4);
    return smx::launch_poly_bank(p->d, p->d_bus, p->d_slots, p->n_pad, (uint32_t)n, p->stream,
                                 no_defer ? nullptr : &p->pend, p->bend_mul);
}

// Whoever is about to read the last block's bus first runs the fold its launch deferred (a no-op when nothing is owed).
static int poly_flush(smx_poly *p) { return smx::launch_poly_flush(&p->pend, p->stream); }

extern "C" int smx_poly_sync(smx_poly *p)
{
    if (!p) return SMX_E_ARG;
    SMX_HIP(hipSetDevice(p->device));
    int rv = poly_flush(p);                          // after a sync the last block's bus holds its sums
    if (rv) return rv;
    SMX_HIP(hipStreamSynchronize(p->stream));
    return SMX_OK;
}

extern "C" int smx_poly_run(smx_poly *p, float *vec_lr, int32_t *bus_lr, int n)
{
    if (!p || n <= 0) { set_error("smx_poly_run: bad args"); return SMX_E_ARG; }
    for (int done = 0; done < n;) {
        const int nf = n - done < 64 ? n - done : 64;
        int rv = smx_poly_run_async(p, nf);
        if (rv) return rv;
        rv = poly_flush(p);
        if (rv) return rv;
        SMX_HIP(hipMemcpyAsync(p->h_bus, p->d_bus, (size_t)nf * 8, hipMemcpyDeviceToHost, p->stream));
        SMX_HIP(hipStreamSynchronize(p->stream));
        if (bus_lr) memcpy(bus_lr + 2 * done, p->h_bus, (size_t)nf * 8);
        if (vec_lr) for (int i = 0; i < 2 * nf; i++) vec_lr[2 * done + i] = bus_to_float(p->h_bus[i]);
        done += nf;
    }
    return SMX_OK;
}

extern "C" int smx_poly_timer_start(smx_poly *p)
{
    if (!p) return SMX_E_ARG;
    SMX_HIP(hipSetDevice(p->device));
    SMX_HIP(hipEventRecord(p->ev_t0, p->stream));
    return SMX_OK;
}

extern "C" int smx_poly_timer_stop(smx_poly *p, float *ms)
{
    if (!p || !ms) return SMX_E_ARG;
    SMX_HIP(hipSetDevice(p->device));
    SMX_HIP(hipEventRecord(p->ev_t1, p->stream));
    SMX_HIP(hipEventSynchronize(p->ev_t1));
    SMX_HIP(hipEventElapsedTime(ms, p->ev_t0, p->ev_t1));
    return SMX_OK;
}


// ---------------------------------------------------------------------------
// note events: the allocator runs on the device (poly_alloc.hip), in event order, without a host sync
// ---------------------------------------------------------------------------
// The staging slot for a batch of up to n events (grown, with a sync, only when a batch is larger than any before).
static int poly_stage(smx_poly *p, size_t n, uint32_t **ops)
{
    if (p->n >= 0x80000000u) { set_error("smx_poly note events: n_voices=%u (< 2^31)", p->n); return SMX_E_RANGE; }
    SMX_HIP(hipSetDevice(p->device));
    if (p->ops_cap < n) {
        SMX_HIP(hipStreamSynchronize(p->stream));
        size_t cap = p->ops_cap ? p->ops_cap : 1024u;
        while (cap < n) cap *= 2;
        for (int i = 0; i < 2; i++) {
            if (p->h_ops[i]) SMX_HIP(hipHostFree(p->h_ops[i]));
            p->h_ops[i] = nullptr;
            SMX_HIP(hipHostMalloc((void **)&p->h_ops[i], cap * 8, hipHostMallocDefault));
            if (!p->ev_stage[i]) SMX_HIP(hipEventCreateWithFlags(&p->ev_stage[i], hipEventDisableTiming));
            p->ev_stage_busy[i] = false;
        }
        if (p->d_ops) SMX_HIP(hipFree(p->d_ops));
        p->d_ops = nullptr;
        SMX_HIP(hipMalloc((void **)&p->d_ops, cap * 8));
        p->ops_cap = cap;
    }
    const int k = p->ev_k;
    if (p->ev_stage_busy[k]) {                               // the copy that last read this slot
        SMX_HIP(hipEventSynchronize(p->ev_stage[k]));
        p->ev_stage_busy[k] = false;
    }
    *ops = p->h_ops[k];
    return SMX_OK;
}

// host-only op kind: all sound off, a kernel of its own between the allocator's launches
enum { OP_SOUND_OFF = 7 };

static inline void put_op(uint32_t *ops, size_t &n, uint32_t kind, int note)
{
    const int m = note % 128;
    ops[2 * n] = (uint32_t)m | kind << 8;
    ops[2 * n + 1] = note_to_inc(m);
    n++;
}

// the op of a note event: a note_off under a down pedal sustains instead
static inline void put_note(smx_poly *p, uint32_t *ops, size_t &n, bool on, int note)
{
    put_op(ops, n, on ? smx::POLY_OP_ON : (p->controllers && p->pedal) ? smx::POLY_OP_SUSTAIN : smx::POLY_OP_OFF, note);
}

static inline bool own_launch(uint32_t kind)
{
    return kind == smx::POLY_OP_RELEASE_SUSTAINED || kind == smx::POLY_OP_OFF_ALL || kind == OP_SOUND_OFF;
}

// The n ops staged in the current slot -> one H2D copy, then launches in order: runs of up to POLY_EV_CAP note ops
// through the allocator (two kernels when the run holds a note_on, one otherwise), and every release-all and
// all-sound-off in a launch of its own.  Stream order puts them after the blocks queued before
// and ahead of the next one; the deferred fold of the last block (PolyPending) touches only its bus and copies,
// never the arrays written here, so it stays owed to the next launch.
static int poly_submit(smx_poly *p, size_t n)
{
    if (n == 0) return SMX_OK;                               // nothing to do: nothing launched
    const int k = p->ev_k;
    const uint32_t *ops = p->h_ops[k];
    SMX_HIP(hipMemcpyAsync(p->d_ops, ops, n * 8, hipMemcpyHostToDevice, p->stream));
    SMX_HIP(hipEventRecord(p->ev_stage[k], p->stream));
    p->ev_stage_busy[k] = true;
    p->ev_k ^= 1;
    for (size_t e0 = 0; e0 < n;) {
        const uint32_t kind0 = ops[2 * e0] >> 8;
        int rv;
        uint32_t ne = 1;
        if (kind0 == OP_SOUND_OFF) {
            rv = smx::launch_poly_sound_off(p->d, p->d_note2voice, p->d_voice_note, p->d_sustained, p->n_pad, p->stream);
        } else {
            bool any_on = false;
            if (!own_launch(kind0)) {
                ne = 0;
                while (e0 + ne < n && ne < (uint32_t)smx::POLY_EV_CAP && !own_launch(ops[2 * (e0 + ne)] >> 8))
                    any_on |= (ops[2 * (e0 + ne++)] >> 8) == smx::POLY_OP_ON;
            }
            rv = smx::launch_poly_alloc(p->d, p->d_note2voice, p->d_voice_note, p->d_sustained, p->d_ops + 2 * e0, ne,
                                        any_on, p->n, p->d_alloc, p->stream);
        }
        if (rv) return rv;
        e0 += ne;
    }
    return SMX_OK;
}

static int poly_note(smx_poly *p, int note, bool on, const char *what)
{
    if (!p) { set_error("%s: null bank", what); return SMX_E_ARG; }
    if (note < 0) { set_error("%s: note %d < 0", what, note); return SMX_E_ARG; }
    uint32_t *ops;
    int rv = poly_stage(p, 1, &ops);
    if (rv) return rv;
    size_t n = 0;
    put_note(p, ops, n, on, note);
    return poly_submit(p, n);
}

extern "C" int smx_poly_note_on(smx_poly *p, int note) { return poly_note(p, note, true, "smx_poly_note_on"); }
extern "C" int smx_poly_note_off(smx_poly *p, int note) { return poly_note(p, note, false, "smx_poly_note_off"); }

extern "C" uint32_t smx_poly_bend_mul(int bend14, int semitones)
{
    const int b = bend14 < 0 ? 0 : bend14 > 16383 ? 16383 : bend14;
    const int r = semitones < 0 ? 0 : semitones > 24 ? 24 : semitones;
    return (uint32_t)llround(65536.0 * exp2((double)r * (b - 8192) / (8192.0 * 12.0)));
}

static void poly_set_bend(smx_poly *p, int bend14, int range)
{
    p->bend14 = bend14;
    p->bend_range = range;
    p->bend_mul = smx_poly_bend_mul(bend14, range);
}

// One 3-byte message -> at most one op (appended at ops[n]); pedal and bend are updated on the host.
// process_midi's dispatch (linux/synth.c:236-258) for 0x90 / 0x80, then, with the controllers on, channel 0's
// CC 64 / 120 / 121 / 123 and pitch bend.  Everything else is ignored.
static void poly_parse(smx_poly *p, const uint8_t *m, uint32_t *ops, size_t &n)
{
    if (m[0] == 0x90) { put_note(p, ops, n, m[2] != 0, m[1]); return; }      // velocity 0: note_off
    if (m[0] == 0x80) { put_note(p, ops, n, false, m[1]); return; }
    if (!p->controllers) return;
    if (m[0] == 0xE0) { poly_set_bend(p, (m[1] & 0x7F) | (m[2] & 0x7F) << 7, p->bend_range); return; }
    if (m[0] != 0xB0) return;
    switch (m[1]) {
    case 64: {                                               // sustain pedal
        const bool down = m[2] >= 64;
        if (down == p->pedal) return;
        p->pedal = down;
        if (!down) put_op(ops, n, smx::POLY_OP_RELEASE_SUSTAINED, 0);
        return;
    }
    case 120: put_op(ops, n, OP_SOUND_OFF, 0); return;      // all sound off
    case 121:                                                // reset all controllers: pedal up, bend to centre
        if (p->pedal) { p->pedal = false; put_op(ops, n, smx::POLY_OP_RELEASE_SUSTAINED, 0); }
        poly_set_bend(p, 8192, p->bend_range);
        return;
    case 123:                                                // all notes off: sustained under a down pedal
        put_op(ops, n, p->pedal ? smx::POLY_OP_SUSTAIN_ALL : smx::POLY_OP_OFF_ALL, 0);
        return;
    default: return;
    }
}

extern "C" int smx_poly_midi_event(smx_poly *p, const uint8_t *msg, size_t size)
{
    if (!p || (size && !msg)) { set_error("smx_poly_midi_event: bad args"); return SMX_E_ARG; }
    if (size != 3) return SMX_OK;
    uint32_t *ops;
    int rv = poly_stage(p, 1, &ops);
    if (rv) return rv;
    size_t n = 0;
    poly_parse(p, msg, ops, n);
    return poly_submit(p, n);
}

extern "C" int smx_poly_midi_events(smx_poly *p, const uint8_t *msgs3, size_t n_events)
{
    if (!p || (n_events && !msgs3)) { set_error("smx_poly_midi_events: bad args"); return SMX_E_ARG; }
    if (n_events == 0) return SMX_OK;
    uint32_t *ops;
    int rv = poly_stage(p, n_events, &ops);
    if (rv) return rv;
    size_t n = 0;
    for (size_t i = 0; i < n_events; i++) poly_parse(p, msgs3 + 3 * i, ops, n);
    return poly_submit(p, n);
}

extern "C" int smx_poly_set_controllers(smx_poly *p, int on)
{
    if (!p) { set_error("smx_poly_set_controllers: null bank"); return SMX_E_ARG; }
    p->controllers = on != 0;
    return SMX_OK;
}

extern "C" int smx_poly_set_bend_range(smx_poly *p, int semitones)
{
    if (!p || semitones < 0 || semitones > 24) { set_error("smx_poly_set_bend_range: semitones=%d (0..24)", semitones); return SMX_E_ARG; }
    poly_set_bend(p, p->bend14, semitones);
    return SMX_OK;
}

extern "C" int smx_poly_read_sustain(smx_poly *p, uint8_t sustained[128])
{
    if (!p || !sustained) { set_error("smx_poly_read_sustain: bad args"); return SMX_E_ARG; }
    SMX_HIP(hipSetDevice(p->device));
    SMX_HIP(hipStreamSynchronize(p->stream));
    SMX_HIP(hipMemcpy(sustained, p->d_sustained, 128, hipMemcpyDeviceToHost));
    return SMX_OK;
}

extern "C" int smx_poly_read_notes(smx_poly *p, int32_t note2voice[128])
{
    if (!p || !note2voice) { set_error("smx_poly_read_notes: bad args"); return SMX_E_ARG; }
    SMX_HIP(hipSetDevice(p->device));
    SMX_HIP(hipStreamSynchronize(p->stream));
    SMX_HIP(hipMemcpy(note2voice, p->d_note2voice, 128 * 4, hipMemcpyDeviceToHost));
    return SMX_OK;
}
