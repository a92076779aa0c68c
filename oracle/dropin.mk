# oracle/dropin.mk -- builds the reference's own programs, unchanged, against the drop-in (include/
# first on the include path, libezrs_hip.so / libezrs_fec.so as the engine).  Run by
# __graft_entry__.build() where the reference tree exists; the binaries land in oracle/_ref/bin/
# (out of git, like the rest of oracle/_ref) and find their libraries relative to themselves
# ($ORIGIN), so the tree may be moved or copied to the GPU box after the build.  The GPU tests
# (tests/test_ref_harness_gpu.py, test_bch_dropin.py, test_rskey_dropin.py, test_ezcod_dropin.py)
# run them.
#
#   rsexercise   rsexercise.C + exercise.H (ezpwd::RS<...>, the reed_solomon<7 params> type surface)
#   rsvalidate   rsvalidate.C: ezpwd::reed_solomon_base codecs on the engine, cross-checked against
#                Phil Karn's CPU libfec (oracle/_ref/libkarn.so, the reference's checker, built from
#                phil-karn/fec-3.0.1.tar.gz by oracle/Makefile)
#   rsspeed      rsspeed.C: the same pairing, timed (single-codeword calls)
#   rstest       phil-karn/rstest.c + exercise.c (x4: char, int, fixed-8, CCSDS), compiled with the
#                tarball's own headers, linked against libezrs_fec.so: Karn's ABI over the engine.
#                exercise.c is compiled with -DDEBUG=1, the reference's own knob that sets 10 trials
#                per (pad, load) class (exercise.c:136-138): rstest.c's Tab asks for up to 100000
#                single-codeword round trips per class, hours of PCIe round trips through a GPU
#   ezcod_gpu    ezcod.C (the ezcod C API over ezpwd::RS<31,31-P>) with tests/cpp/ezcod_driver.cpp
#   rskey_test, rspwd_test
#                the reference's self-checking tests of ezpwd/corrector over RS<31,..> / RS<63,..>;
#                include/ezpwd/corrector defuses corrector's sibling #include "rs"
#   bchsimple, bchclassic
#                the reference's BCH programs (ezpwd::BCH<255,239,2> and the classic bch API)
#
# The tarball is unpacked (headers only are used) into a temporary directory outside the repository,
# with the reference's int-symbol patch applied exactly as phil-karn/GNUmakefile:43-52 prepares it,
# and the directory is deleted when the recipe ends.  Nothing from the reference is copied into the
# repository: the compiler reads its sources in place.
REFERENCE ?= $(error pass REFERENCE=<path of the reference tree>)
HERE     := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT      := $(abspath $(HERE)..)
OUT       := $(HERE)_ref/bin
LIB       := $(ROOT)/ezpwd-reed-solomon_amd/lib
KARNLIB   := $(HERE)_ref
CXXF      := -std=c++17 -O2 -w -I$(ROOT)/include -I$(REFERENCE)/c++ -I$(REFERENCE)
TGZ       := $(REFERENCE)/phil-karn/fec-3.0.1.tar.gz
KEX       := $(REFERENCE)/phil-karn/exercise.c
DROPIN    := $(wildcard $(ROOT)/include/ezpwd_amd/* $(ROOT)/include/ezpwd/*)
# run-time library paths relative to oracle/_ref/bin
RP_LIB    := -Wl,-rpath,'$$ORIGIN/../../../ezpwd-reed-solomon_amd/lib'
RP_KARN   := -Wl,-rpath,'$$ORIGIN/..'

.PHONY: all FORCE
all: $(OUT)/rsexercise $(OUT)/.karn_stamp $(OUT)/ezcod_gpu $(OUT)/rskey_test $(OUT)/rspwd_test \
     $(OUT)/bchsimple $(OUT)/bchclassic
FORCE:

# the stamp stands for three binaries: if any of them is gone (a partial clean of bin), rebuild
KARN_BINS    := $(OUT)/rsvalidate $(OUT)/rsspeed $(OUT)/rstest
KARN_MISSING := $(filter-out $(wildcard $(KARN_BINS)),$(KARN_BINS))

$(OUT)/rsexercise: $(REFERENCE)/rsexercise.C $(REFERENCE)/exercise.H $(DROPIN)
	@mkdir -p $(OUT)
	g++ $(CXXF) -o $@ $< -L$(LIB) -lezrs_hip $(RP_LIB)

$(OUT)/ezcod_gpu: $(ROOT)/tests/cpp/ezcod_driver.cpp $(REFERENCE)/ezcod.C $(DROPIN)
	@mkdir -p $(OUT)
	g++ $(CXXF) -o $@ $(ROOT)/tests/cpp/ezcod_driver.cpp $(REFERENCE)/ezcod.C -L$(LIB) -lezrs_hip $(RP_LIB)

$(OUT)/rskey_test $(OUT)/rspwd_test: $(OUT)/%: $(REFERENCE)/%.C $(DROPIN)
	@mkdir -p $(OUT)
	g++ $(CXXF) -o $@ $< -L$(LIB) -lezrs_hip $(RP_LIB)

$(OUT)/bchsimple $(OUT)/bchclassic: $(OUT)/%: $(REFERENCE)/%.C $(DROPIN)
	@mkdir -p $(OUT)
	g++ -std=c++17 -O2 -I$(ROOT)/include -I$(REFERENCE)/c++ -o $@ $< -L$(LIB) -lezrs_hip $(RP_LIB)

# rsvalidate, rsspeed and rstest: the programs that need libfec's headers, built in one recipe around
# one temporary unpack of the tarball
$(OUT)/.karn_stamp: $(REFERENCE)/rsvalidate.C $(REFERENCE)/rsspeed.C $(REFERENCE)/phil-karn/rstest.c $(KEX) \
                    $(TGZ) $(DROPIN) $(LIB)/libezrs_fec.so $(HERE)dropin.mk \
                    $(if $(KARN_MISSING),FORCE)
	@mkdir -p $(OUT)
	T=$$(mktemp -d) && ( set -e; \
	  tar xzf $(TGZ) -C $$T; \
	  cd $$T/fec-3.0.1 && for p in $(REFERENCE)/phil-karn/fec-3.0.1*.patch; do patch -s -p1 < $$p; done; \
	  ln -sfn fec-3.0.1 $$T/fec; \
	  KF="-I$(REFERENCE)/phil-karn -I$$T"; \
	  g++ $(CXXF) $$KF -o $(OUT)/rsvalidate $(REFERENCE)/rsvalidate.C -L$(LIB) -lezrs_hip -L$(KARNLIB) -lkarn \
	      $(RP_LIB) $(RP_KARN); \
	  g++ $(CXXF) $$KF -o $(OUT)/rsspeed $(REFERENCE)/rsspeed.C -L$(LIB) -lezrs_hip -L$(KARNLIB) -lkarn \
	      $(RP_LIB) $(RP_KARN); \
	  KC="-O2 -w -I$$T/fec-3.0.1 $$KF"; \
	  gcc $$KC -c -o $$T/rstest.o $(REFERENCE)/phil-karn/rstest.c; \
	  gcc $$KC -DDEBUG=1 -c -o $$T/ex_char.o $(KEX); \
	  gcc $$KC -DDEBUG=1 -DBIGSYM -c -o $$T/ex_int.o $(KEX); \
	  gcc $$KC -DDEBUG=1 -DFIXED -c -o $$T/ex_8.o $(KEX); \
	  gcc $$KC -DDEBUG=1 -DCCSDS -c -o $$T/ex_ccsds.o $(KEX); \
	  g++ -o $(OUT)/rstest $$T/rstest.o $$T/ex_char.o $$T/ex_int.o $$T/ex_8.o $$T/ex_ccsds.o \
	      -L$(LIB) -lezrs_fec -lezrs_hip $(RP_LIB) ); rc=$$?; rm -rf $$T; exit $$rc
	touch $@
