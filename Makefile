# convenience targets; __graft_entry__.build() does the same from Python
HIPCC ?= hipcc
LIB    = quadsim_amd/csrc/libquadsim_hip.so
SRC    = quadsim_amd/csrc/quadsim_hip.hip
HDR    = $(filter-out quadsim_amd/csrc/dynplan_%.hpp,$(wildcard quadsim_amd/csrc/*.hpp)) include/quadsim.h
# the second library (include/quadsim_dyn.h): its own translation unit, same flags
DYNLIB = quadsim_amd/csrc/libquadsim_dyn.so
DYNSRC = quadsim_amd/csrc/dynplan.hip
DYNHDR = $(wildcard quadsim_amd/csrc/dynplan_*.hpp) quadsim_amd/csrc/quadsim_device.hpp include/quadsim_dyn.h

all: lib oracle

lib: $(LIB) $(DYNLIB)
$(LIB): $(SRC) $(HDR)
	$(HIPCC) -std=c++20 -O3 -fno-slp-vectorize -ffp-contract=on --offload-arch=gfx950 -fPIC -shared -Wno-unused-result $(SRC) -lhsa-runtime64 -o $@

$(DYNLIB): $(DYNSRC) $(DYNHDR)
	$(HIPCC) -std=c++20 -O3 -fno-slp-vectorize -ffp-contract=on --offload-arch=gfx950 -fPIC -shared -Wno-unused-result $(DYNSRC) -o $@

oracle:
	$(MAKE) -C oracle

test-cpu: all
	python -m pytest tests -q -m "not gpu"

test-gpu: all
	python -m pytest tests -q -m gpu

bench: all
	python bench.py

clean:
	rm -f $(LIB) $(DYNLIB) oracle/libqso.so oracle/*.o

.PHONY: all lib oracle test-cpu test-gpu bench clean
