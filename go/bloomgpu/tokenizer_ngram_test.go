package bloomgpu

import (
	"fmt"
	"testing"
)

// Tokenizer.Func with an n-gram width: the worked values of bloomgpu.h's definition (the same table the host mirror and the
// device are pinned to in tests/test_tokenizer_ngram_spec.py); Validate refuses widths other than 0, 2, 3, 4.  Host only.
func TestTokenizerNgramFunc(t *testing.T) {
	def := func(n int) Tokenizer {
		return Tokenizer{Separators: " \t\n\v\f\r", UnicodeSpace: true, Lower: true, Ngram: n}
	}
	cases := []struct {
		tok  Tokenizer
		in   string
		want []string
	}{
		{def(3), "Hello ok", []string{"hel", "ell", "llo", "ok"}},
		{def(2), "héllo", []string{"hé", "él", "ll", "lo"}},
		{def(4), "abc abcd abcde", []string{"abc", "abcd", "abcd", "bcde"}},
		{Tokenizer{Ngram: 3}, "ab cd", []string{"ab ", "b c", " cd"}},
		{def(3), "\u212aELVIN", []string{"kel", "elv", "lvi", "vin"}},
		{def(3), "-1.5e-3", []string{"-1.", "1.5", ".5e", "5e-", "e-3"}},
		{def(3), "true", []string{"tru", "rue"}},
		{def(2), "ȺȺb", []string{"ⱥⱥ", "ⱥb"}},
		{Tokenizer{Ngram: 4}, "x\U0001F600\U0001F601\U0001F602\U0001F603y", []string{"x\U0001F600\U0001F601\U0001F602",
			"\U0001F600\U0001F601\U0001F602\U0001F603", "\U0001F601\U0001F602\U0001F603y"}},
		{Tokenizer{Separators: ",", Ngram: 2}, "a\xffb", []string{"a\xff", "\xffb"}},
		{def(0), "Hello ok", []string{"hello", "ok"}},
		{def(3), "", nil},
	}
	for _, c := range cases {
		got := c.tok.Func()(c.in)
		if fmt.Sprintf("%q", got) != fmt.Sprintf("%q", c.want) {
			t.Errorf("%+v(%q) = %q, want %q", c.tok, c.in, got, c.want)
		}
	}
	for _, n := range []int{2, 3, 4} {
		if err := def(n).Validate(); err != nil {
			t.Errorf("Validate(Ngram %d): %v", n, err)
		}
	}
	for _, n := range []int{-1, 1, 5, 6, 7, 8} {
		if def(n).Validate() == nil {
			t.Errorf("Validate(Ngram %d) accepted", n)
		}
	}
	if ct := def(3).c(); uint32(ct.flags) != 3|3<<8 || ct.reserved != 0 {
		t.Errorf("C form of a trigram spec: flags %#x reserved %d", uint32(ct.flags), uint32(ct.reserved))
	}
}
