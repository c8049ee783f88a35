# TEST INFRASTRUCTURE: indirect_main, a stand-alone program linked against this directory's sanitizer build (Makefile), the runtime linked statically.
.DEFAULT_GOAL := indirect
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
$(B)/rtw_device.o: $(wildcard $(C)/rtw_*_kernels.h)     # (the Makefile's own rule does not list them all: see features.mk)
indirect: $(HERE)indirect_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $(B)/indirect_main -lz -lpthread -ldl
