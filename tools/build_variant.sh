#!/bin/bash
# usage: build_variant.sh <out .so name> [extra flags]  -- builds the product library with extra -D flags into
# voronoirt_amd/<out>, from the sources and with the flags of voronoirt_amd/build.py.
#   VRT_VARIANT_UNITS="a.hip b.cpp": only these units of csrc/, linked against the libvrt_hip.so beside the result, which
#   supplies everything else (tests/test_tessellate_device.py: vrt_tessellate.hip with a lowered face capacity)
set -e
out=$1; shift
cd "$(dirname "$0")/.."
S=${VRT_VARIANT_UNITS:-$(python3 -c "from voronoirt_amd import build; print(' '.join(build.SOURCES))")}
link=""
[ -n "$VRT_VARIANT_UNITS" ] && link="-L voronoirt_amd -Wl,-rpath,\$ORIGIN -lvrt_hip"
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result -I include -I voronoirt_amd/csrc -o voronoirt_amd/$out "$@" $(for s in $S; do echo voronoirt_amd/csrc/$s; done) $link -lpthread -ldl
