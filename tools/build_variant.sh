#!/bin/bash
# diagnostic builds of the RX kernel objects: tools/build_variant.sh NAME [-DFLAG ...] -> t41_sdr_amd/abl/libt41rx_NAME.so
# (select with T41RX_LIB=...; the host objects are the product's).  Every variant is built with -DT41RX_EXPERIMENT=1
# (rx_experiments.hpp): a variant with -DT41RX_STAMP / -DT41RX_PIPE_STAT / -DT41RX_CLK reports itself and t41rx_create()
# refuses it unless T41RX_ALLOW_EXPERIMENT=1 is in the environment -- the tools that use such builds set it.
# Which objects are recompiled and which are the product's is the Makefile's list (print-rxk-objs / print-host-objs).
set -e
NAME=$1; shift
cd "$(dirname "$0")/../t41_sdr_amd/csrc"
RXK_OBJS=$(make -s print-rxk-objs)
HOST_OBJS=$(make -s print-host-objs)
make -s -j8 $HOST_OBJS
mkdir -p ../abl
B=/tmp/rxk_$NAME
rm -rf "$B"; mkdir -p "$B"
PIDS=()
for OBJ in $RXK_OBJS; do
  TU=${OBJ%.o}
  hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -fno-slp-vectorize -I../../include -DT41RX_EXPERIMENT=1 "$@" -c $TU.hip -o $B/$TU.o &
  PIDS+=($!)
done
FAIL=0
for P in "${PIDS[@]}"; do wait "$P" || FAIL=1; done
[ $FAIL = 0 ] || { echo "build_variant.sh: a kernel object of $NAME failed to compile" >&2; exit 1; }
hipcc -shared -fPIC --offload-arch=gfx950 $B/*.o $HOST_OBJS -o ../abl/libt41rx_$NAME.so
