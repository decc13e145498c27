// What a persistent launch waits for at the per-device gate and what it records there afterwards (gate.hip, PersistGate): a pure
// function of the launch's slots (rnn_plan.h: RnnLaunch), the CUs of the ring windows recorded last, the device's CUs and whether the
// whole-device turn word exists.  Host-only and without a HIP include, like rnn_plan.h: gate.hip executes the masks; `make asan` builds
// the same header for the CPU (tools/asan/host_fuzz.cpp gate, tests/test_asan_host.py).
#pragma once
#include "rnn_plan.h"

namespace dsmi {

// The part of the gate the decision reads: CUs of the window last recorded on each ring slot (it may still be running).
struct DeviceGateState { int ring_cus[kRingSlots] = {0, 0, 0, 0, 0}; };

// Bit i of `lanes`: the event of lane slot i; bit i of `ring`: the event of ring slot i.
struct DeviceGateWait {
    unsigned lanes = 0, ring = 0;
    bool full = false;         // wait for the whole-device launch recorded last
    bool acquire = false;      // take the device turn (turn_acquire_kernel), behind the event waits
};
struct DeviceGateRecord {
    unsigned lanes = 0, ring = 0;
    bool full = false;         // record the whole-device event
    bool release = false;      // give the device turn back (turn_release_kernel), in front of the event records
    DeviceGateState after;
};

inline DeviceGateWait gate_plan_wait(const DeviceGateState& st, const RnnLaunch& L, int n_cus, bool have_turn) {
    DeviceGateWait w;
    const int first = L.slot0, n = L.nslots;
    if (L.gate == GATE_RING) {
        // `n` windows of the ring kernel, L.cus CUs each, on ring slots [first, first + n).  Slots are counted per model (n_cus / cus of
        // ITS geometry), but they index one set of events per device: two models of different widths in one process could otherwise
        // be admitted side by side beyond the device (H = 800: 50 CUs on slots 0..4, H = 896: 56 CUs on slots 0..3 -- slot 4 at 50
        // CUs beside four windows at 56 is 274 CUs), and windows that are not all resident spin to their timeout.  So a launch also
        // waits for as many OTHER slots as it takes for the windows that may still run plus its own to fit the device.
        int others = 0;
        for (int i = 0; i < kRingSlots; ++i) {
            if (i >= first && i < first + n) w.ring |= 1u << i;
            else others += st.ring_cus[i];
        }
        for (int i = 0; i < kRingSlots && others + n * L.cus > n_cus; ++i) {
            if ((i >= first && i < first + n) || !st.ring_cus[i]) continue;
            w.ring |= 1u << i;
            others -= st.ring_cus[i];
        }
        // behind every launch of the other kernels (the two families never share the device)
        w.lanes = (1u << kMaxLanes) - 1;
        w.full = true;
        return w;
    }
    // the lane slots [first, first + width) this launch needs (gate_first), and every ring window
    for (int i = first; i < first + n && i < kMaxLanes; ++i) w.lanes |= 1u << i;
    w.ring = (1u << kRingSlots) - 1;
    // whole device: behind the slot-sized launches by events, among themselves by the lock
    if (n >= kMaxLanes && have_turn) w.acquire = true;
    else w.full = true;
    return w;
}

inline DeviceGateRecord gate_plan_record(const DeviceGateState& st, const RnnLaunch& L, bool have_turn) {
    DeviceGateRecord r;
    r.after = st;
    const int first = L.slot0, n = L.nslots;
    if (L.gate == GATE_RING) {
        for (int i = first; i < first + n && i < kRingSlots; ++i) {
            r.ring |= 1u << i;
            r.after.ring_cus[i] = L.cus;
        }
        return r;
    }
    if (n >= kMaxLanes && have_turn) {
        r.release = r.full = true;
        return r;
    }
    for (int i = first; i < first + n && i < kMaxLanes; ++i) r.lanes |= 1u << i;
    return r;
}

}  // namespace dsmi
