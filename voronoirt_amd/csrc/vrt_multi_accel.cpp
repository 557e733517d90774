// The C entries of include/voronoirt_multi_accel.h: Ng acceleration of the multi-device line session.  They are the whole of
// the companion library libvrt_hip_multi_accel.so, which links libvrt_hip.so and forwards to vrt_multi.cpp: libvrt_hip.so
// itself exports exactly what voronoirt.h declares, and voronoirt.h declares no acceleration entry of vrt_multi_lambda_*.
#include "vrt_internal.h"

extern "C" {

int vrt_multi_lambda_set_acceleration(vrt_multi_lambda *s, int order, int start, int period)
{
    return vrt::multi_lambda_set_acceleration(s, order, start, period);
}

int vrt_multi_lambda_last_acceleration(const vrt_multi_lambda *s, int *applied, double sums[5], double coeffs[2])
{
    return vrt::multi_lambda_last_acceleration(s, applied, sums, coeffs);
}

}  // extern "C"
