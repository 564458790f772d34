// cancel.hpp -- the host state machine of hm_cancel (ABI 1.18): one cancel
// flag per context, who may set it, who clears it, and the record of the last
// cancelled call.  No HIP here: device.cpp points `flag` at the context's pinned
// word, and tests/test_cancel_host.py builds this header alone under
// ThreadSanitizer with a plain word in its place.
//
//   the call's thread (ctx->mu held)        any other thread
//   begin(family)  flag = 0, in flight      request()  in flight ? flag = 1, stamp : nothing
//   seen()         after every wait / readback, before a control word is read
//   observed(n)    first sight of the flag: n launches were in flight
//   finish(rc)     not in flight; rc == HM_ERR_CANCELLED: the record
//
// `mu` (cancel_mu) orders begin, request and finish, so a request lands on the
// call that is in flight or on none: nothing is remembered between calls, and a
// flag set after a call's last seen() is cleared by the next call's begin()
// before that call enqueues anything.  The flag is the only word the device
// reads (the relay wave, cancel_relay.hpp): it is set before the device can see
// it and cleared only here, by the call's own thread, at call start.
#pragma once
#include <stdint.h>

#include <chrono>
#include <mutex>

#include "../../include/hipminer.h"

namespace hm {

struct CancelState {
    std::mutex mu;              // never held across a HIP call
    uint32_t* flag = nullptr;   // pinned, mapped, coherent host word (device.cpp)
    bool in_flight = false;     // a cancellable call is between begin() and finish()
    int family = 0;             // HM_CANCEL_FAMILY_* of that call
    int32_t launches = 0;       // observed(): launches in flight then
    std::chrono::steady_clock::time_point stamp{};  // request(): the flag store
    hm_cancel_stats stats{};

    void begin(int fam) {
        std::lock_guard<std::mutex> g(mu);
        __atomic_store_n(flag, 0u, __ATOMIC_RELEASE);
        in_flight = true;
        family = fam;
        launches = 0;
    }
    // hm_cancel: 1 = a cancellable call was in flight and is signalled.
    int request() {
        std::lock_guard<std::mutex> g(mu);
        if (!in_flight) return 0;
        if (!__atomic_load_n(flag, __ATOMIC_RELAXED)) {
            __atomic_store_n(flag, 1u, __ATOMIC_RELEASE);
            stamp = std::chrono::steady_clock::now();
        }
        ++stats.cancels;
        return 1;
    }
    bool seen() const { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) != 0; }
    void observed(int inflight) {
        std::lock_guard<std::mutex> g(mu);
        launches = inflight;
    }
    void finish(int rc) {
        std::lock_guard<std::mutex> g(mu);
        in_flight = false;
        if (rc != HM_ERR_CANCELLED) return;
        stats.latency_ms = std::chrono::duration<double, std::milli>(
                               std::chrono::steady_clock::now() - stamp)
                               .count();
        stats.launches_in_flight = launches;
        stats.family = family;
        ++stats.cancelled_calls;
    }
    hm_cancel_stats read() {
        std::lock_guard<std::mutex> g(mu);
        return stats;
    }
};

}  // namespace hm
