# Another build of libsdr beside the shipped one (never shipped itself): libsdr_<name>.so from the
# sources as they stand, with any extra compiler flags, e.g.
#   bash tools/build_dbg.sh O2 -O2
# then run a script with SDR_LIB=real-time-software-defined-radio_amd/libsdr_O2.so.  To compare
# against another commit, build that commit's library from a clean export of it and copy it here
# under such a name (tools/ab_dbg.sh, tools/rx_digest.py, tools/blocks_digest.py).
set -e
NAME=$1
shift
cd "$(dirname "$0")/../real-time-software-defined-radio_amd/csrc"
O=../_build_$NAME
mkdir -p $O
for f in $(sed -n 's/^SRCS *= *//p' Makefile); do            # the sources the shipped library is made of
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-inline-asm "$@" -c $f -o $O/${f%.hip}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libsdr_$NAME.so $O/*.o
