// The per-device gate that keeps persistent recurrent kernels from sharing CUs, and the dense kernels' token beside it (gate.hip).
// What a launch waits for and records is decided in gate_plan.h; this is what the rest of the library sees of the gate.
#pragma once
#include "common.h"

#include <mutex>

struct PersistGate;      // (gate.hip; named here only for GateTurn's pointer)

// true when this process may run persistent kernels on `device` (the cross-process lock file)
bool persist_process_lock(int device);
// the home lane of the next handle on `device` (rnn_plan.h: gate_first)
int persist_next_lane(int device);

// One turn at the device's gate: wait -> the caller's launch(es) -> record, under the gate's mutex, so that the turns of two host
// threads with two handles / streams always chain one behind the other.  Several launches under one turn (RnnLaunch::join):
// record() publishes the launch given to wait() -- joined launches share the first launch's gate and slots (rnn_plan.h).
// The mutex is let go at record() or at the end of the scope, whichever comes first.
class GateTurn {
public:
    // take the mutex and make stream `s` wait for what launch `L` needs on a device of `n_cus` CUs
    void wait(int device, hipStream_t s, const dsmi::RnnLaunch& L, int n_cus);
    // publish that launch on its slots and let the mutex go
    void record();
    // Not a turn: the mutex alone, no wait and no record, let go only at the end of the scope -- no other launch of this process
    // can start meanwhile (the stamp diagnostics, which run on a drained device)
    void hold(int device);
private:
    PersistGate* g_ = nullptr;
    std::unique_lock<std::mutex> lk_;
    hipStream_t s_ = nullptr;
    dsmi::RnnLaunch l_;
};

// One forward at a time in a dense kernel (see dense_enter_kernel): enter in front of the kernels of `scope`, leave behind them.
// Holds nothing unless the token is on, the caller keeps two batches or more in flight and the scope is one that runs behind the
// token (DSMI_DEBUG_DENSE_SCOPE in the experiments build).  No destructor: leave() is a launch on the stream and belongs at its
// place in the launch order, so the caller calls it -- and must not return between the two.
enum DenseScope { DENSE_CONV_STACK, DENSE_CONV_LAYER, DENSE_GEMM };
int dense_token_limit();      // forwards that may be in a dense kernel at a time; 0: the token is off (DSMI_DENSE_TOKENS, hardware queues)
class DenseHold {
public:
    DenseHold(int device, int inflight, DenseScope scope, hipStream_t s);      // enters
    void leave();
private:
    unsigned* sem_ = nullptr;
    hipStream_t s_ = nullptr;
};
