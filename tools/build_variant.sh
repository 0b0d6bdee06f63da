#!/bin/bash
# diagnostic builds of the RX kernel objects: tools/build_variant.sh NAME [-DFLAG ...] -> t41_sdr_amd/abl/libt41rx_NAME.so
# (select with T41RX_LIB=...).  The library is built by the product's Makefile, every object by the product's rule, into an
# object directory of its own (t41_sdr_amd/abl/obj_NAME); only KFLAGS differs, so only the Makefile's RXK_OBJS do.  Every
# variant is built with -DT41RX_EXPERIMENT=1 (rx_experiments.hpp): a variant with -DT41RX_STAMP / -DT41RX_PIPE_STAT /
# -DT41RX_CLK reports itself and t41rx_create() refuses it unless T41RX_ALLOW_EXPERIMENT=1 is in the environment -- the
# tools that use such builds set it.
set -e
NAME=$1; shift
exec make -s -j8 -C "$(dirname "$0")/../t41_sdr_amd/csrc" OBJDIR=../abl/obj_$NAME OUT=../abl/libt41rx_$NAME.so KFLAGS="-DT41RX_EXPERIMENT=1 $*" lib
