// The member protocol of the multi-device object (vrt_multi.cpp): one piece of work per device, each on a host thread of
// its own, and ONE report.  Every entry of vrt_multi_* that touches the devices goes through on_members; nothing else
// in the library starts a thread per device.  A member is anything with `int device`, `int rc`, `std::string err` and
// `std::mutex &plan_mutex()`.  Inline host code, like vrt_source_store.h: tests/probes/line_block_main.cpp compiles it
// against a fake runtime, with ThreadSanitizer too.
#pragma once

#include "vrt_internal.h"

namespace vrt {

enum {
    kLockPlan = 1,      // the body runs with the member's plan mutex held
    kNoDevice = 2,      // the member's device is NOT made current first (vrt_multi_create: it is not known to exist yet)
};

inline bool every_member(int) { return false; }     // (a `skip` that skips nobody)

// body(d, member) -> rc on every member d that skip(d) does not leave out: the member's device made current, its plan
// locked if asked for.  The error text of a failing body is thread-local, so the worker copies it into the member before
// it ends.  After the join: a body that threw is VRT_ENOMEM; otherwise the first failing member in device order is
// reported as "device N: <its text>" with its code.
template <typename Member, typename Skip, typename Body>
int on_members(std::vector<Member> &m, int options, Skip skip, Body body)
{
    auto work = [&](int d) {
        Member &me = m[(size_t)d];
        me.rc = VRT_OK;
        if (skip(d)) return;
        if (!(options & kNoDevice) && hipSetDevice(me.device) != hipSuccess) me.rc = fail(VRT_ENODEVICE, "hipSetDevice failed");
        else if (options & kLockPlan) {
            std::lock_guard<std::mutex> plock(me.plan_mutex());
            me.rc = body(d, me);
        } else
            me.rc = body(d, me);
        if (me.rc) me.err = vrt_last_error();
    };
    if (!run_workers((int)m.size(), work)) return fail(VRT_ENOMEM, "out of host memory in a device worker");
    for (const Member &me : m)
        if (me.rc) return fail(me.rc, "device " + std::to_string(me.device) + ": " + me.err);
    return VRT_OK;
}

}  // namespace vrt
