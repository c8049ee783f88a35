# TEST INFRASTRUCTURE: material_main, a stand-alone program linked against the objects of this directory's sanitizer build (Makefile) and run directly.
# The sanitizers' runtime is linked into the program statically (the objects are the same either way), so it needs nothing from its environment.
.DEFAULT_GOAL := material
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
material: $(B)/material_main
$(B)/material_main: $(HERE)material_main.cpp $(OBJS) $(HERE)../../include/rtwin.h
	$(CXX) $(filter-out -shared-libasan,$(FLAGS)) -I$(HERE)../../include $< $(OBJS) -o $@ -lz -lpthread -ldl
