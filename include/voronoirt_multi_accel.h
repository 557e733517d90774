/* voronoirt_multi_accel.h -- Ng acceleration of the multi-device line session (vrt_multi_lambda_*).  voronoirt.h includes
 * this file at its end; a caller includes voronoirt.h.  The two entries are NOT exported by libvrt_hip.so but by the
 * companion library libvrt_hip_multi_accel.so, built beside it, which links it through its own directory: a C caller
 * links both (-lvrt_hip_multi_accel -lvrt_hip), a dlopen caller opens libvrt_hip.so, then the companion beside it.
 * After an error of vrt_multi_lambda_iterate that arose while an ACCEPTED step rewrote the down-order copies, the
 * session's S is inconsistent: every further vrt_multi_lambda_iterate is refused (VRT_ENODEVICE) until
 * vrt_multi_lambda_set_state has replaced S.
 *
 * vrt_multi_lambda_set_acceleration / vrt_multi_lambda_last_acceleration carry the contract of the single-device entries
 * (voronoirt.h, vrt_lambda_set_acceleration) word for word: order 0 = off (default) or 2; the first step is due after
 * iterate number `start` (>= 4), the next ones after every `period` further iterates (>= 4); anything else is VRT_EINVAL,
 * with order 0 start and period are ignored; callable between any two iterates (a due iterate whose three predecessors were
 * not all recorded takes no step); order 0 frees the history.  vrt_multi_lambda_iterate returns what it returns without
 * acceleration, the scalar of the PLAIN update; populations, R, γ and J are not extrapolated.  *applied = 1 taken, 0 none
 * due, -1 due but rejected; sums / coeffs (either may be NULL) valid unless 0.  A session that never calls the setter
 * allocates and runs nothing extra and returns what it returned before, bit for bit.  Argument errors (a NULL session, a
 * bad order, start or period) are reported before any device is touched.
 *
 * What is specific to a session whose S is split over the devices:
 * Every device (member) that holds wavelengths keeps three copies of ITS block of S (three extra S blocks per device),
 * recorded at the iterates at which the single-device session records them; a member without wavelengths (more devices
 * than wavelengths) keeps nothing and takes no part.  On a due iterate every member forms the five sums over the physical
 * entries of its block; the session's sums are the members' added on the host in member order ((s_0 + s_1) + s_2) + ...,
 * never in the order of completion, so a session gives the same bits run after run; vrt_multi_lambda_last_acceleration
 * reports these sums and the ONE (a, b) made of them.  Every member applies that (a, b) to its block into its oldest
 * history buffer; the step is taken ALL OR NOTHING: only if the coefficients are valid and every member reports every
 * x_acc finite and > 0 do the buffers become the members' S (the down-order copies rewritten from them); otherwise no
 * member's S changes and *applied = -1.  No collective is involved: five doubles per member come to the host, two go back.
 * If one member cannot allocate its history, all members' histories are released, the order is 0, the error is returned
 * and the session goes on as a plain one.  vrt_multi_lambda_set_state drops every member's history; the settings and the
 * iterate counter stay.  The setter takes the locks vrt_multi_lambda_iterate takes. */
#ifndef VORONOIRT_MULTI_ACCEL_H
#define VORONOIRT_MULTI_ACCEL_H

#include "voronoirt.h"

#ifdef __cplusplus
extern "C" {
#endif

int vrt_multi_lambda_set_acceleration(vrt_multi_lambda *s, int order, int start, int period);
int vrt_multi_lambda_last_acceleration(const vrt_multi_lambda *s, int *applied, double sums[5], double coeffs[2]);

#ifdef __cplusplus
}
#endif
#endif /* VORONOIRT_MULTI_ACCEL_H */
