// Test harness (TEST INFRASTRUCTURE ONLY): the environment switches' one reader
// (crdt_amd/csrc/yc_switches.h, included alone). Every argument NAME=VALUE is put into the
// environment with setenv (NAME=@n or @n+tail: a value of n characters '0', then the tail, for the
// long-value cases; a bare NAME: the empty string), then read_switches() runs and every field is printed as field=value on one
// line, in the table's order. tests/test_switches.py holds the expected lines, written out by hand.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "yc_switches.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t eq = a.find('=');
    std::string v = eq == std::string::npos ? "" : a.substr(eq + 1);
    if (!v.empty() && v[0] == '@') {
      const size_t plus = v.find('+');
      v = std::string(std::stoul(v.substr(1, plus - 1)), '0') + (plus == std::string::npos ? "" : v.substr(plus + 1));
    }
    setenv(a.substr(0, eq).c_str(), v.c_str(), 1);
  }
  const yc::Switches s = yc::read_switches();
  const char* sep = "";
#define X(type, field, name, parse, dflt, when, what) \
  printf("%s%s=%llu", sep, #field, (unsigned long long)s.field); \
  sep = " ";
  YC_SWITCHES(X)
#undef X
  printf("\n");
  return 0;
}
