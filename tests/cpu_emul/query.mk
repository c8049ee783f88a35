# TEST INFRASTRUCTURE: query_main, a stand-alone program linked against the objects of this directory's sanitizer build (Makefile) and run directly.
# The sanitizers' runtime is linked into the program statically (the objects are the same either way), so it needs nothing from its environment.
.DEFAULT_GOAL := query
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
$(B)/rtw_device.o: $(C)/rtw_query_kernels.h
query: $(B)/query_main
$(B)/query_main: $(HERE)query_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $@ -lz -lpthread -ldl
