# convenience targets; __graft_entry__.build() does the same from Python
PYTHON ?= python

all: lib oracle

# all the libraries, with the flags, sources and dependencies of quadsim_amd/_lib.py (HIPCC overrides the compiler there too)
lib:
	$(PYTHON) -c "from quadsim_amd import _lib; _lib.build_library(verbose=True)"

oracle:
	$(MAKE) -C oracle

test-cpu: all
	$(PYTHON) -m pytest tests -q -m "not gpu"

test-gpu: all
	$(PYTHON) -m pytest tests -q -m gpu

bench: all
	$(PYTHON) bench.py

clean:
	rm -f quadsim_amd/csrc/libquadsim_*.so oracle/libqso.so oracle/*.o

.PHONY: all lib oracle test-cpu test-gpu bench clean
