# Host build of csrc/sequence.hpp (test infrastructure; see sequences.cpp):  make -C tests/hostsim -f sequences.mk
CXX ?= g++
CXXFLAGS ?= -O2 -g -std=c++17 -fPIC -Wall -Wno-unknown-pragmas -ffp-contract=off
HDR := ../../mallorn-astrophysics_amd/csrc/sequence.hpp ../../mallorn-astrophysics_amd/csrc/wave.hpp

all: libsequences.so

# the template on the one-lane policy, as tests/test_sequences_cpu.py compiles it
libsequences.so: sequences.cpp $(HDR)
	$(CXX) $(CXXFLAGS) -shared -o $@ sequences.cpp -lm

# the stand-alone program under AddressSanitizer and UBSan
sequences_check: sequences.cpp $(HDR)
	$(CXX) $(CXXFLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -DSEQUENCES_MAIN -o $@ sequences.cpp -lm

clean:
	rm -f libsequences.so sequences_check
